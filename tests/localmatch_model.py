"""The specification of the batched SearchLocalPoints (include/orbx_localmatch.h) as the reference's loop
(ORBmatcher::SearchByProjection(Frame&, map points), src/ORBmatcher.cc:43-141, Nleft == -1), in numpy float32 / float64 scalars: one
operation at a time, for a whole batch.  Slow and plain on purpose."""
import math

import numpy as np

F = np.float32
COLS, ROWS = 64, 48
TH_HIGH = 100


def _round(v):
    """C's round() of a float32 value: halves away from zero."""
    v = float(v)
    return math.floor(v + 0.5) if v >= 0 else math.ceil(v - 0.5)


def grid_inverses(bounds):
    """mfGridElementWidthInv, mfGridElementHeightInv (src/Frame.cc:153-160), float32."""
    min_x, min_y, max_x, max_y = (F(v) for v in bounds)
    with np.errstate(all="ignore"):
        return F(64) / F(max_x - min_x), F(48) / F(max_y - min_y)


def cell_of(x, y, bounds):
    """Frame::PosInGrid (src/Frame.cc:725-735) -> ix * 48 + iy, or -1 for a feature in no cell."""
    inv_w, inv_h = grid_inverses(bounds)
    with np.errstate(all="ignore"):
        px, py = F(F(F(x) - F(bounds[0])) * inv_w), F(F(F(y) - F(bounds[1])) * inv_h)
    if not (math.isfinite(px) and math.isfinite(py)):
        return -1
    ix, iy = _round(px), _round(py)
    return -1 if ix < 0 or ix >= COLS or iy < 0 or iy >= ROWS else ix * ROWS + iy


def assign_grid(kps, bounds):
    """mGrid flattened: 3072 lists of feature indices, each in ascending index (Frame::AssignFeaturesToGrid, src/Frame.cc:385-416)."""
    cells = [[] for _ in range(COLS * ROWS)]
    for i in range(len(kps)):
        c = cell_of(kps["x"][i], kps["y"][i], bounds)
        if c >= 0:
            cells[c].append(i)
    return cells


def radius_of(view_cos, level, scale_factors, th):
    """RadiusByViewingCos (:214-220) against the double literal, th when it is not 1.0, the level's scale: float32, rounded once each."""
    r = F(2.5) if float(F(view_cos)) > 0.998 else F(4.0)
    if float(F(th)) != 1.0:
        r = F(r * F(th))
    return F(r * F(scale_factors[level]))


def features_in_area(kps, cells, bounds, x, y, r, min_level, max_level):
    """Frame::GetFeaturesInArea (src/Frame.cc:657-723): the indices in the reference's order."""
    min_x, min_y = F(bounds[0]), F(bounds[1])
    inv_w, inv_h = grid_inverses(bounds)
    x, y, r = F(x), F(y), F(r)
    out = []
    if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(r)):
        return out                                               # the documented limit: undefined in the reference
    n_min_x = max(0, math.floor(F(F(F(x - min_x) - r) * inv_w)))
    if n_min_x >= COLS:
        return out
    n_max_x = min(COLS - 1, math.ceil(F(F(F(x - min_x) + r) * inv_w)))
    if n_max_x < 0:
        return out
    n_min_y = max(0, math.floor(F(F(F(y - min_y) - r) * inv_h)))
    if n_min_y >= ROWS:
        return out
    n_max_y = min(ROWS - 1, math.ceil(F(F(F(y - min_y) + r) * inv_h)))
    if n_max_y < 0:
        return out
    check_levels = min_level > 0 or max_level >= 0
    for ix in range(n_min_x, n_max_x + 1):
        for iy in range(n_min_y, n_max_y + 1):
            for i in cells[ix * ROWS + iy]:
                if check_levels:
                    octave = int(kps["octave"][i])
                    if octave < min_level:
                        continue
                    if max_level >= 0 and octave > max_level:
                        continue
                distx, disty = F(F(kps["x"][i]) - x), F(F(kps["y"][i]) - y)
                if abs(distx) < r and abs(disty) < r:
                    out.append(i)
    return out


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def candidates(kps, desc, uright, cells, bounds, p, pdesc, scale_factors, th):
    """One in-view point (a record of POINT_DTYPE) -> [(index, distance, octave)] in walk order, the stereo gate applied (:96-101); the kp_obs
    test is the caller's."""
    if not (math.isfinite(p["proj_x"]) and math.isfinite(p["proj_y"]) and math.isfinite(p["view_cos"])):
        return []
    level = int(p["level"])
    radius = radius_of(p["view_cos"], level, scale_factors, th)
    out = []
    for i in features_in_area(kps, cells, bounds, p["proj_x"], p["proj_y"], radius, level - 1, level):
        if uright is not None and F(uright[i]) > 0:
            er = abs(F(F(p["proj_xr"]) - F(uright[i])))
            if er > radius:
                continue
        out.append((i, hamming(pdesc[p["point"]], desc[i]), int(kps["octave"][i])))
    return out


def decide(cands, obs_row, nn_ratio):
    """The scan over the candidates that are not hidden (:86-115) and the acceptance (:117-130) -> the keypoint, or -1."""
    best, level, best2, level2, idx = 256, -1, 256, -1, -1
    for i, dist, octave in cands:
        if obs_row[i] > 0:
            continue
        if dist < best:
            best2, best, level2, level, idx = best, dist, level, octave, i
        elif dist < best2:
            level2, best2 = octave, dist
    if best <= TH_HIGH:
        if level == level2 and F(best) > F(F(nn_ratio) * F(best2)):
            return -1
        if level != level2 or F(best) <= F(F(nn_ratio) * F(best2)):
            return idx
    return -1


def malformed(K, cap, mcap, M, nlevels, counts, f, nmp, row):
    if not (0 <= f < K) or not (0 <= nmp <= mcap) or not (0 <= int(counts[f, 0]) <= cap):
        return True
    live = row[:nmp][row[:nmp]["in_view"] != 0]
    return bool(((live["level"] < 0) | (live["level"] >= nlevels) | (live["point"] < 0) | (live["point"] >= M)).any())


def search(kps, desc, counts, uright, bounds, frames, mp, nmp, pdesc, scale_factors, th, nn_ratio, kp_obs, chain=True):
    """The whole call on host arrays of the ABI's layout -> (nmatches [B], kp_match [B, cap], kp_obs [B, cap] after the call,
    taken [B, mcap]: the keypoint each point was accepted with, -1 without).  A malformed item gives -1, a row of -1 and kp_obs as it was.
    chain=False: every point sees the kp_obs row as it arrived (the chain-free arg-min; not the specification)."""
    K, cap = kps.shape
    B, mcap = mp.shape
    M, nlevels = len(pdesc), len(scale_factors)
    nmatches, match, obs = np.zeros(B, np.int32), np.full((B, cap), -1, np.int32), np.array(kp_obs, np.int32).reshape(B, cap).copy()
    taken = np.full((B, mcap), -1, np.int32)
    grids = {}
    for b in range(B):
        f, m = int(frames[b]), int(nmp[b])
        if malformed(K, cap, mcap, M, nlevels, counts, f, m, mp[b]):
            nmatches[b] = -1
            continue
        n = int(counts[f, 0])
        if f not in grids:
            grids[f] = assign_grid(kps[f, :n], bounds[f])
        ur = None if uright is None else uright[f, :n]
        seen = obs[b].copy()
        for q in range(m):
            p = mp[b, q]
            if p["in_view"] == 0:
                continue
            i = decide(candidates(kps[f, :n], desc[f, :n], ur, grids[f], bounds[f], p, pdesc, scale_factors, th), obs[b] if chain else seen, nn_ratio)
            taken[b, q] = i
            if i >= 0:
                match[b, i], obs[b, i] = q, p["obs"]
                nmatches[b] += 1
    return nmatches, match, obs, taken
