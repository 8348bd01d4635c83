"""The specification of the batched relocalization and Sim3 matchers (include/orbx_projmatch.h) as the reference's loops
(ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist), src/ORBmatcher.cc:1889-2010, kind 0, and
SearchByProjection(pKF, Scw, vpPoints[, vpPointsKFs], vpMatched[, vpMatchedKF], th, ratioHamming), :427-532 and :534-646, kind 1), in numpy
float32 scalars: one operation at a time, for a whole batch.  Slow and plain on purpose.  The frame grid and Frame::GetFeaturesInArea are
tests/localmatch_model.py's; the bin and the three maxima tests/lastmatch_model.py's."""
import math

import numpy as np

from tests.lastmatch_model import HISTO_LENGTH, rot_bin, three_maxima  # noqa: F401
from tests.localmatch_model import F, assign_grid, cell_of, features_in_area, grid_inverses, hamming  # noqa: F401

TH_LOW = 50
RELOC, SIM3 = 0, 1


def radius_of(th, level, scale_factors):
    """:489, :602, :1937: float32, rounded once."""
    return F(F(th) * F(scale_factors[level]))


def max_dist_sim3(ratio):
    """:523, :636: TH_LOW * ratioHamming, an int converted to float times a float."""
    return F(F(TH_LOW) * F(ratio))


def level_range(kind, level):
    """(qmin, qmax) of the equivalent filtered window: :1939 for kind 0; for kind 1 the test of :509 / :622."""
    return (level - 1, level + 1) if kind == RELOC else (level - 1, level)


def area(kps, cells, bounds, kind, u, v, radius, level):
    """Kind 0: Frame::GetFeaturesInArea(u, v, radius, level - 1, level + 1).  Kind 1: KeyFrame::GetFeaturesInArea(u, v, radius), no level
    filter (min_level = 0, max_level = -1: bCheckLevels false), then the walk's own test."""
    if kind == RELOC:
        return features_in_area(kps, cells, bounds, u, v, radius, level - 1, level + 1)
    out = []
    for i in features_in_area(kps, cells, bounds, u, v, radius, 0, -1):
        kp_level = int(kps["octave"][i])
        if kp_level < level - 1 or kp_level > level:
            continue
        out.append(i)
    return out


def candidates(kps, desc, cells, bounds, p, pdesc, scale_factors, item):
    """One valid point (a record of POINT_DTYPE) of `item` (a record of ITEM_DTYPE) -> [(index, distance)] in walk order; the taken test is
    the caller's."""
    if not (math.isfinite(p["u"]) and math.isfinite(p["v"])):
        return []
    level = int(p["level"])
    radius = radius_of(item["th"], level, scale_factors)
    return [(i, hamming(pdesc[p["point"]], desc[i])) for i in area(kps, cells, bounds, int(item["kind"]), p["u"], p["v"], radius, level)]


def malformed(K, cap, mcap, M, nlevels, counts, item, npts, row):
    f = int(item["frame"])
    if not (0 <= f < K) or not (0 <= npts <= mcap) or not (0 <= int(counts[f, 0]) <= cap):
        return True
    if not (0 <= int(item["kind"]) <= 1) or not math.isfinite(item["th"]):
        return True
    live = row[:npts][row[:npts]["valid"] != 0]
    return bool(((live["level"] < 0) | (live["level"] >= nlevels) | (live["point"] < 0) | (live["point"] >= M)).any())


def chain(lists, points, kps, item, check_orientation, taken_in, cap):
    """Steps 4 to 6 for one item over its points' candidate lists (lists[q]: [(index, distance)] or None for a point that is skipped) ->
    (nmatches, kp_match [cap], bound [npts]: the keypoint each point was accepted with, -1 without, bins [npts]: its histogram bin, -1
    without an entry)."""
    match = np.full(cap, -1, np.int32)
    taken = np.zeros(cap, bool) if taken_in is None else np.array(taken_in, np.uint8).reshape(cap) != 0
    bound, bins = np.full(len(lists), -1, np.int32), np.full(len(lists), -1, np.int32)
    histogram = check_orientation and int(item["kind"]) == RELOC
    hist = [[] for _ in range(HISTO_LENGTH)]
    limit = F(item["max_dist"])
    nmatches = 0
    for q, cands in enumerate(lists):
        if cands is None:
            continue
        best, idx = 256, -1
        for i, dist in cands:
            if taken[i]:                                          # :504, :1952
                continue
            if dist < best:
                best, idx = dist, i
        if idx < 0 or not F(best) <= limit:                       # no candidate is never accepted; a NaN limit accepts nothing
            continue
        match[idx], taken[idx] = q, True
        nmatches += 1
        bound[q] = idx
        if histogram:
            k = rot_bin(points[q]["angle"], kps[idx]["angle"])
            bins[q] = k
            if k >= 0:
                hist[k].append(idx)
    if histogram:
        keep = three_maxima([len(h) for h in hist])
        for k in range(HISTO_LENGTH):
            if k in keep:
                continue
            for idx in hist[k]:
                match[idx] = -2
                nmatches -= 1
    return nmatches, match, bound, bins


def search(kps, desc, counts, bounds, items, points, npts, pdesc, scale_factors, check_orientation, kp_taken, lists_of=None):
    """The whole call on host arrays of the ABI's layout -> (nmatches [B], kp_match [B, cap], bound [B, mcap], bins [B, mcap]).  A
    malformed item gives -1 and a row of -1.  lists_of(b, f, n, q, p) -> [(index, distance)]: another source of a live point's candidates
    (the oracle's lists) in place of this file's."""
    K, cap = kps.shape
    B, mcap = points.shape
    M, nlevels = len(pdesc), len(scale_factors)
    nmatches, match = np.zeros(B, np.int32), np.full((B, cap), -1, np.int32)
    bound, bins = np.full((B, mcap), -1, np.int32), np.full((B, mcap), -1, np.int32)
    grids = {}
    for b in range(B):
        it, m = items[b], int(npts[b])
        if malformed(K, cap, mcap, M, nlevels, counts, it, m, points[b]):
            nmatches[b] = -1
            continue
        f = int(it["frame"])
        n = int(counts[f, 0])
        if f not in grids and lists_of is None:
            grids[f] = assign_grid(kps[f, :n], bounds[f])
        lists = []
        for q in range(m):
            p = points[b, q]
            if p["valid"] == 0:
                lists.append(None)
            elif lists_of is not None:
                lists.append(lists_of(b, f, n, q, p))
            else:
                lists.append(candidates(kps[f, :n], desc[f, :n], grids[f], bounds[f], p, pdesc, scale_factors, it))
        nmatches[b], match[b], bound[b, :m], bins[b, :m] = chain(lists, points[b], kps[f], it, check_orientation,
                                                                 None if kp_taken is None else kp_taken[b], cap)
    return nmatches, match, bound, bins


def oracle_lists(kps, desc, bounds, scale_factors, item, row, pdesc, kp_skip=None):
    """oracle.pyoracle.window_search_grid's lists for a row's live points -> {q: [(index, distance)]}: the frame's grid assigned with its
    float bounds, the level range of the item's kind as (qmin, qmax).  Not part of the model: what the tests hold it (and the GPU) to."""
    from oracle import pyoracle as po
    live = np.nonzero((row["valid"] != 0) & np.isfinite(row["u"]) & np.isfinite(row["v"]))[0]
    if len(live) == 0 or len(kps) == 0:
        return {int(q): [] for q in live}
    inv_w, inv_h = grid_inverses(bounds)
    cs, ci = po.assign_grid(kps, F(bounds[0]), F(bounds[1]), inv_w, inv_h)
    grid = dict(min_x=float(bounds[0]), min_y=float(bounds[1]), inv_w=float(inv_w), inv_h=float(inv_h), cell_start=cs, cell_idx=ci)
    level = row["level"][live]
    rng = [level_range(int(item["kind"]), int(l)) for l in level]
    qr = np.array([radius_of(item["th"], int(l), scale_factors) for l in level], np.float32)
    w = po.window_search_grid(kps, desc, grid, row["u"][live], row["v"][live], qr, [a for a, _ in rng], [b for _, b in rng], pdesc[row["point"][live]],
                              kp_skip=kp_skip)
    rp = w["row_ptr"]
    return {int(q): list(zip(w["cand"][rp[j]:rp[j + 1]].tolist(), w["dist"][rp[j]:rp[j + 1]].tolist())) for j, q in enumerate(live)}
