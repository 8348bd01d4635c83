"""The specification of the batched two-camera rig matchers (include/orbx_rigmatch.h) as the reference's loops with Nleft != -1
(ORBmatcher::SearchByProjection(Frame&, map points), src/ORBmatcher.cc:43-212, and SearchByProjection(CurrentFrame, LastFrame),
:1676-1886), in numpy float32 / float64 scalars: sequential and literal, one operation at a time, candidate lists in the reference's walk
order.  Slow and plain on purpose.  Every function also returns a trace: what each point did, for the tests that hold a constructed batch
to its claims."""
import math

import numpy as np

from tests.localmatch_model import F, TH_HIGH, assign_grid, features_in_area, hamming, radius_of

HISTO_LENGTH = 30


def _finite(*v):
    return all(math.isfinite(float(x)) for x in v)


def _malformed_side(K, cap_l, cap_r, counts_l, counts_r, f):
    return not (0 <= f < K) or not (0 <= int(counts_l[f, 0]) <= cap_l) or not (0 <= int(counts_r[f, 0]) <= cap_r)


def local_malformed(side, mcap, M, nlevels, f, nmp, row):
    K, cap_l, cap_r = side["kps_l"].shape[0], side["kps_l"].shape[1], side["kps_r"].shape[1]
    if _malformed_side(K, cap_l, cap_r, side["counts_l"], side["counts_r"], f) or not (0 <= nmp <= mcap):
        return True
    r = row[:nmp]
    in_l, in_r = r["in_view"] != 0, r["in_view_r"] != 0
    if (in_l & ((r["level"] < 0) | (r["level"] >= nlevels))).any() or (in_r & ((r["level_r"] < -1) | (r["level_r"] >= nlevels))).any():
        return True
    if ((in_l | in_r) & ((r["point"] < 0) | (r["point"] >= M))).any():
        return True
    nl, nr = int(side["counts_l"][f, 0]), int(side["counts_r"][f, 0])
    l2r, r2l = side["l2r"][f, :nl], side["r2l"][f, :nr]
    return bool(((l2r < -1) | (l2r >= nr)).any() or ((r2l < -1) | (r2l >= nl)).any())


def _top2(cands, base, obs_row):
    """The scan of :84-120 / :164-190 over the candidates whose slot is open -> best, level, best2, level2, idx."""
    best, level, best2, level2, idx = 256, -1, 256, -1, -1
    for i, dist, octave in cands:
        if obs_row[base + i] > 0:
            continue
        if dist < best:
            best2, best, level2, level, idx = best, dist, level, octave, i
        elif dist < best2:
            level2, best2 = octave, dist
    return best, level, best2, level2, idx


def _window(kps, desc, cells, bounds, x, y, radius, lo, hi, d):
    if not _finite(x, y):
        return []
    return [(i, hamming(d, desc[i]), int(kps["octave"][i])) for i in features_in_area(kps, cells, bounds, x, y, radius, lo, hi)]


def search_local(side, frames, mp, nmp, pdesc, scale_factors, th, nn_ratio, kp_obs):
    """Entry 1 on host arrays of the ABI's layout; side: dict(kps_l, desc_l, counts_l, kps_r, desc_r, counts_r, l2r, r2l, bounds).
    -> (nmatches [B], kp_match [B, slots], kp_obs [B, slots] after the call, trace): trace[b][q] = dict(left=..., right=..., lists=(nl,
    nr)) with left / right one of None (block not run), "empty", "none" (no open candidate or bestDist > 100), "ratio" (the `continue`),
    or ("accept", slot, cross slot or None, cross slot was hidden)."""
    cap_l, cap_r = side["kps_l"].shape[1], side["kps_r"].shape[1]
    slots = cap_l + cap_r
    B, mcap = mp.shape
    M, nlevels = len(pdesc), len(scale_factors)
    nmatches, match = np.zeros(B, np.int32), np.full((B, slots), -1, np.int32)
    obs = np.array(kp_obs, np.int32).reshape(B, slots).copy()
    trace, grids = [None] * B, {}
    ratio = F(nn_ratio)
    for b in range(B):
        f, m = int(frames[b]), int(nmp[b])
        if local_malformed(side, mcap, M, nlevels, f, m, mp[b]):
            nmatches[b] = -1
            continue
        nl, nr = int(side["counts_l"][f, 0]), int(side["counts_r"][f, 0])
        kl, kr, dl, dr = side["kps_l"][f, :nl], side["kps_r"][f, :nr], side["desc_l"][f, :nl], side["desc_r"][f, :nr]
        bounds = side["bounds"][f]
        if f not in grids:
            grids[f] = assign_grid(kl, bounds), assign_grid(kr, bounds)
        gl, gr = grids[f]
        l2r, r2l = side["l2r"][f], side["r2l"][f]
        o, tr = obs[b], {}
        trace[b] = tr

        def write(slot, q, p):
            match[b, slot], o[slot] = q, p["obs"]
            nmatches[b] += 1

        for q in range(m):
            p = mp[b, q]
            if p["in_view"] == 0 and p["in_view_r"] == 0:
                continue
            t = tr[q] = dict(left=None, right=None, lists=[0, 0])
            if p["in_view"] != 0:
                cands = []
                if _finite(p["proj_x"], p["proj_y"], p["view_cos"]):
                    level = int(p["level"])
                    cands = _window(kl, dl, gl, bounds, p["proj_x"], p["proj_y"], radius_of(p["view_cos"], level, scale_factors, th), level - 1, level,
                                    pdesc[p["point"]])
                t["lists"][0] = len(cands)
                t["left"] = "empty"
                if cands:
                    best, level1, best2, level2, idx = _top2(cands, 0, o)
                    t["left"] = "none"
                    if best <= TH_HIGH:
                        if level1 == level2 and F(best) > F(ratio * F(best2)):
                            t["left"] = "ratio"
                            continue                              # :126
                        if level1 != level2 or F(best) <= F(ratio * F(best2)):
                            write(idx, q, p)
                            cross, hid = None, False
                            if l2r[idx] != -1:
                                cross = cap_l + int(l2r[idx])
                                hid = bool(o[cross] > 0)
                                write(cross, q, p)
                            t["left"] = ("accept", idx, cross, hid)
            if p["in_view_r"] != 0 and p["level_r"] != -1:
                cands = []
                if _finite(p["proj_xr"], p["proj_yr"], p["view_cos_r"]):
                    level = int(p["level_r"])
                    cands = _window(kr, dr, gr, bounds, p["proj_xr"], p["proj_yr"], radius_of(p["view_cos_r"], level, scale_factors, 1.0), level - 1,
                                    level, pdesc[p["point"]])
                t["lists"][1] = len(cands)
                t["right"] = "empty"
                if not cands:
                    continue
                best, level1, best2, level2, idx = _top2(cands, cap_l, o)
                t["right"] = "none"
                t["right_hidden"] = [cap_l + i for i, _, _ in cands if o[cap_l + i] > 0]
                if best <= TH_HIGH:
                    if level1 == level2 and F(best) > F(ratio * F(best2)):
                        t["right"] = "ratio"
                        continue
                    cross, hid = None, False
                    if r2l[idx] != -1:
                        cross = int(r2l[idx])
                        hid = bool(o[cross] > 0)
                        write(cross, q, p)
                    write(cap_l + idx, q, p)
                    t["right"] = ("accept", cap_l + idx, cross, hid)
    return nmatches, match, obs, trace


def last_malformed(side, mcap, M, nlevels, item, nlast, row):
    K, cap_l, cap_r = side["kps_l"].shape[0], side["kps_l"].shape[1], side["kps_r"].shape[1]
    f = int(item["frame"])
    if _malformed_side(K, cap_l, cap_r, side["counts_l"], side["counts_r"], f) or not (0 <= nlast <= mcap):
        return True
    if not (0 <= int(item["direction"]) <= 2) or not math.isfinite(float(item["th"])):
        return True
    live = row[:nlast][row[:nlast]["valid"] != 0]
    return bool(((live["octave"] < 0) | (live["octave"] >= nlevels) | (live["point"] < 0) | (live["point"] >= M)).any())


def rot_bin(angle_a, angle_b):
    """:1784-1790; -1 when the bin falls outside 0 .. 30 (the reference asserts; the entry is then never removed)."""
    rot = F(F(angle_a) - F(angle_b))
    if rot < 0.0:
        rot = F(rot + F(360.0))
    v = float(F(rot * F(F(1.0) / F(HISTO_LENGTH))))
    if not math.isfinite(v):
        return -1
    r = math.floor(v + 0.5) if v >= 0 else math.ceil(v - 0.5)
    if not (0 <= r <= HISTO_LENGTH):
        return -1
    return 0 if r == HISTO_LENGTH else r


def three_maxima(hist):
    """ComputeThreeMaxima (:2012-2053) on the bins' sizes."""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(hist):
        if s > max1:
            max3, max2, max1, ind3, ind2, ind1 = max2, max1, s, ind2, ind1, i
        elif s > max2:
            max3, max2, ind3, ind2 = max2, s, ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if F(max2) < F(F(0.1) * F(max1)):
        ind2 = ind3 = -1
    elif F(max3) < F(F(0.1) * F(max1)):
        ind3 = -1
    return ind1, ind2, ind3


def search_last(side, items, points, nlast, pdesc, scale_factors, check_orientation, kp_obs):
    """Entry 2 -> (nmatches, kp_match, kp_obs, trace): trace[b] = dict(points={q: dict(left=, right=, lists=)}, entries=[(q, slot, bin)],
    kept=(ind1, ind2, ind3)); left / right: None, "empty", "none" or ("accept", slot)."""
    cap_l, cap_r = side["kps_l"].shape[1], side["kps_r"].shape[1]
    slots = cap_l + cap_r
    B, mcap = points.shape
    M, nlevels = len(pdesc), len(scale_factors)
    nmatches, match = np.zeros(B, np.int32), np.full((B, slots), -1, np.int32)
    obs = np.array(kp_obs, np.int32).reshape(B, slots).copy()
    trace, grids = [None] * B, {}
    for b in range(B):
        it, m = items[b], int(nlast[b])
        if last_malformed(side, mcap, M, nlevels, it, m, points[b]):
            nmatches[b] = -1
            continue
        f, direction, th = int(it["frame"]), int(it["direction"]), F(it["th"])
        nl, nr = int(side["counts_l"][f, 0]), int(side["counts_r"][f, 0])
        kl, kr, dl, dr = side["kps_l"][f, :nl], side["kps_r"][f, :nr], side["desc_l"][f, :nl], side["desc_r"][f, :nr]
        bounds = side["bounds"][f]
        if f not in grids:
            grids[f] = assign_grid(kl, bounds), assign_grid(kr, bounds)
        gl, gr = grids[f]
        o = obs[b]
        tr = trace[b] = dict(points={}, entries=[], kept=None)
        for q in range(m):
            p = points[b, q]
            if p["valid"] == 0:
                continue
            octave = int(p["octave"])
            radius = F(th * F(scale_factors[octave]))
            lo, hi = ((octave, -1), (0, octave))[direction - 1] if direction else (octave - 1, octave + 1)
            t = tr["points"][q] = dict(left="empty", right=None, lists=[0, 0])
            cands = _window(kl, dl, gl, bounds, p["u"], p["v"], radius, lo, hi, pdesc[p["point"]])
            t["lists"][0] = len(cands)
            if not cands:
                continue                                          # :1735
            for cam, base, kps in ((0, 0, kl), (1, cap_l, kr)):
                if cam:
                    cands = _window(kr, dr, gr, bounds, p["u_r"], p["v_r"], radius, lo, hi, pdesc[p["point"]])
                    t["lists"][1] = len(cands)
                best, idx = 256, -1
                for i, dist, _ in cands:
                    if o[base + i] > 0:
                        continue
                    if dist < best:
                        best, idx = dist, i
                name = "right" if cam else "left"
                t[name] = "none" if cands else "empty"
                if best <= TH_HIGH:
                    slot = base + idx
                    match[b, slot], o[slot] = q, p["obs"]
                    nmatches[b] += 1
                    t[name] = ("accept", slot)
                    if check_orientation:
                        tr["entries"].append((q, slot, rot_bin(p["angle"], kps["angle"][idx])))
        if check_orientation:
            hist = [0] * HISTO_LENGTH
            for _, _, bin_ in tr["entries"]:
                if bin_ >= 0:
                    hist[bin_] += 1
            kept = tr["kept"] = three_maxima(hist)
            for _, slot, bin_ in tr["entries"]:
                if bin_ >= 0 and bin_ not in kept:
                    match[b, slot], o[slot] = -2, -1
                    nmatches[b] -= 1
    return nmatches, match, obs, trace
