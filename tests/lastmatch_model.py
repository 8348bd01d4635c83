"""The specification of the batched frame-to-last-frame matcher (include/orbx_lastmatch.h) as the reference's loop
(ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono), src/ORBmatcher.cc:1676-1885, Nleft == -1), in numpy float32 scalars:
one operation at a time, for a whole batch.  Slow and plain on purpose.  The frame grid and Frame::GetFeaturesInArea are
tests/localmatch_model.py's."""
import math

import numpy as np

from tests.localmatch_model import F, _round, assign_grid, cell_of, features_in_area, grid_inverses, hamming  # noqa: F401

TH_HIGH = 100
HISTO_LENGTH = 30


def level_range(direction, octave):
    """:1728-1733 -> (minLevel, maxLevel) of GetFeaturesInArea."""
    if direction == 1:
        return octave, -1
    if direction == 2:
        return 0, octave
    return octave - 1, octave + 1


def radius_of(th, octave, scale_factors):
    """:1724, float32, rounded once."""
    return F(F(th) * F(scale_factors[octave]))


def gate_ur(u, mbf, invz):
    """:1753: a float32 product, then a float32 subtraction."""
    with np.errstate(all="ignore"):
        return F(F(u) - F(F(mbf) * F(invz)))


def gate_ur_fused(u, mbf, invz):
    """What an FMA would give: the product exact (float64 holds a product of two float32 exactly), one rounding."""
    return F(float(F(u)) - float(F(mbf)) * float(F(invz)))


def rot_bin(angle_a, angle_b):
    """:1784-1790: the bin, or -1 where the reference asserts."""
    with np.errstate(all="ignore"):
        rot = F(F(angle_a) - F(angle_b))
        if rot < 0.0:
            rot = F(rot + F(360.0))
        r = F(rot * F(F(1.0) / F(HISTO_LENGTH)))
    if not math.isfinite(r):
        return -1
    b = _round(r)
    if b == HISTO_LENGTH:
        b = 0
    return b if 0 <= b < HISTO_LENGTH else -1


def three_maxima(counts):
    """ComputeThreeMaxima (src/ORBmatcher.cc:2012-2053) on the bins' sizes -> (ind1, ind2, ind3)."""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(counts):
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


def candidates(kps, desc, uright, cells, bounds, p, pdesc, scale_factors, item):
    """One valid point (a record of POINT_DTYPE) of `item` (a record of ITEM_DTYPE) -> [(index, distance)] in walk order, the stereo gate
    applied (:1751-1757); the kp_obs test is the caller's."""
    if not (math.isfinite(p["u"]) and math.isfinite(p["v"])):
        return []
    octave = int(p["octave"])
    radius = radius_of(item["th"], octave, scale_factors)
    lo, hi = level_range(int(item["direction"]), octave)
    out = []
    for i in features_in_area(kps, cells, bounds, p["u"], p["v"], radius, lo, hi):
        if uright is not None and F(uright[i]) > 0:
            with np.errstate(all="ignore"):
                er = abs(F(gate_ur(p["u"], item["mbf"], p["invz"]) - F(uright[i])))
            if er > radius:
                continue
        out.append((i, hamming(pdesc[p["point"]], desc[i])))
    return out


def malformed(K, cap, mcap, M, nlevels, counts, item, nlast, row):
    f = int(item["frame"])
    if not (0 <= f < K) or not (0 <= nlast <= mcap) or not (0 <= int(counts[f, 0]) <= cap):
        return True
    if not (0 <= int(item["direction"]) <= 2) or not math.isfinite(item["th"]):
        return True
    live = row[:nlast][row[:nlast]["valid"] != 0]
    return bool(((live["octave"] < 0) | (live["octave"] >= nlevels) | (live["point"] < 0) | (live["point"] >= M)).any())


def search(kps, desc, counts, uright, bounds, items, points, nlast, pdesc, scale_factors, check_orientation, kp_obs):
    """The whole call on host arrays of the ABI's layout -> (nmatches [B], kp_match [B, cap], kp_obs [B, cap] after the call,
    taken [B, mcap]: the keypoint each point was accepted with, -1 without, bins [B, mcap]: its histogram bin, -1 without an entry).
    A malformed item gives -1, a row of -1 and kp_obs as it was."""
    K, cap = kps.shape
    B, mcap = points.shape
    M, nlevels = len(pdesc), len(scale_factors)
    nmatches, match, obs = np.zeros(B, np.int32), np.full((B, cap), -1, np.int32), np.array(kp_obs, np.int32).reshape(B, cap).copy()
    taken, bins = np.full((B, mcap), -1, np.int32), np.full((B, mcap), -1, np.int32)
    grids = {}
    for b in range(B):
        it, m = items[b], int(nlast[b])
        if malformed(K, cap, mcap, M, nlevels, counts, it, m, points[b]):
            nmatches[b] = -1
            continue
        f = int(it["frame"])
        n = int(counts[f, 0])
        if f not in grids:
            grids[f] = assign_grid(kps[f, :n], bounds[f])
        ur = None if uright is None else uright[f, :n]
        hist = [[] for _ in range(HISTO_LENGTH)]
        for q in range(m):
            p = points[b, q]
            if p["valid"] == 0:
                continue
            best, idx = 256, -1
            for i, dist in candidates(kps[f, :n], desc[f, :n], ur, grids[f], bounds[f], p, pdesc, scale_factors, it):
                if obs[b, i] > 0:
                    continue
                if dist < best:
                    best, idx = dist, i
            if best <= TH_HIGH:
                match[b, idx], obs[b, idx] = q, p["obs"]
                nmatches[b] += 1
                taken[b, q] = idx
                if check_orientation:
                    k = rot_bin(p["angle"], kps[f, idx]["angle"])
                    bins[b, q] = k
                    if k >= 0:
                        hist[k].append(idx)
        if check_orientation:
            keep = three_maxima([len(h) for h in hist])
            for k in range(HISTO_LENGTH):
                if k in keep:
                    continue
                for idx in hist[k]:
                    match[b, idx], obs[b, idx] = -2, -1
                    nmatches[b] -= 1
    return nmatches, match, obs, taken, bins
