"""ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:648-763) in plain Python, arranged as the kernel of liborbx_initmatch.so is
(include/orbx_initmatch.h): first every query's candidate list in the frame grid's order with every candidate's Hamming distance (nothing
here depends on the order of the queries), then the chain over the precomputed distances, then the rotation filter.  Float arithmetic is
float32, one operation at a time."""
from __future__ import annotations

import math

import numpy as np

COLS, ROWS = 64, 48
INT_MAX = 2 ** 31 - 1
TH_LOW = 50
F = np.float32
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def _round(v) -> int:
    """std::round: halves away from zero (exact in double for a float32 of this size)."""
    v = float(v)
    if math.isnan(v) or math.isinf(v):
        return -(2 ** 31)
    return int(math.copysign(math.floor(abs(v) + 0.5), v))


def rot_bin(a1, a2) -> int:
    rot = F(a1) - F(a2)
    if rot < 0.0:
        rot = F(rot + F(360.0))
    b = _round(F(rot * (F(1.0) / F(30))))
    return 0 if b == 30 else b


def build_grid(kps2, bounds):
    """Phase A, F2's side: the level-0 keypoints inside the grid as sorted keys (cell << 16 | index) -- cells x-major, then y, then
    ascending index -- and the first sorted position of every cell."""
    minx, miny, maxx, maxy = (F(b) for b in bounds)
    inv_w, inv_h = F(COLS) / F(maxx - minx), F(ROWS) / F(maxy - miny)
    keys = []
    for i in range(len(kps2)):
        if int(kps2["octave"][i]) != 0:
            continue
        px, py = _round(F(F(kps2["x"][i]) - minx) * inv_w), _round(F(F(kps2["y"][i]) - miny) * inv_h)
        if 0 <= px < COLS and 0 <= py < ROWS:
            keys.append(((px * ROWS + py) << 16) | i)
    keys = np.array(sorted(keys), np.int64)
    cstart = np.searchsorted(keys, np.arange(COLS * ROWS + 1, dtype=np.int64) << 16, side="left")
    return keys, cstart, (minx, miny, inv_w, inv_h)


def window(x, y, r, keys, cstart, geo, kps2):
    """GetFeaturesInArea(x, y, r, 0, 0) (src/Frame.cc:657-723) over the sorted keys: the candidates in the reference's order."""
    minx, miny, inv_w, inv_h = geo
    x, y, r = F(x), F(y), F(r)

    def cell(v) -> int:
        v = float(v)
        return 0 if math.isnan(v) else int(max(min(v, 2.0 ** 31 - 1), -2.0 ** 31))
    x0 = max(0, cell(np.floor(F(F(x - minx) - r) * inv_w)))
    if x0 >= COLS:
        return []
    x1 = min(COLS - 1, cell(np.ceil(F(F(x - minx) + r) * inv_w)))
    if x1 < 0:
        return []
    y0 = max(0, cell(np.floor(F(F(y - miny) - r) * inv_h)))
    if y0 >= ROWS:
        return []
    y1 = min(ROWS - 1, cell(np.ceil(F(F(y - miny) + r) * inv_h)))
    if y1 < 0 or y1 < y0:
        return []
    runs = [keys[cstart[ix * ROWS + y0]:cstart[ix * ROWS + y1 + 1]] for ix in range(x0, x1 + 1)]   # a column's cells are neighbours
    idx = (np.concatenate(runs) & 0xFFFF).astype(np.int64)
    if not len(idx):
        return []
    inside = (np.abs(kps2["x"][idx].astype(F) - x) < r) & (np.abs(kps2["y"][idx].astype(F) - y) < r)
    return idx[inside].tolist()


def search_for_initialization(kps1, desc1, kps2, desc2, bounds, prev_xy, window_size=100, nn_ratio=0.9, check_ori=True, stats=None):
    """-> (nmatches, vnMatches12 [n1] int32, the updated vbPrevMatched [n1, 2] float32).  `prev_xy` None: F1's own keypoint positions, and
    the third result is None.  `stats` (a dict) receives skipped_taken (candidates skipped because an earlier query holds them at least as
    closely), steals, removed (matches the rotation filter dropped) and single_candidate (acceptances against the INT_MAX start)."""
    n1, n2 = len(kps1), len(kps2)
    d1, d2 = np.ascontiguousarray(desc1, np.uint8).reshape(-1, 32), np.ascontiguousarray(desc2, np.uint8).reshape(-1, 32)
    st = dict(skipped_taken=0, steals=0, removed=0, single_candidate=0)
    centres = np.stack([kps1["x"], kps1["y"]], 1).astype(F) if prev_xy is None else np.asarray(prev_xy, F).reshape(n1, 2)

    # ---- phase A: lists and distances
    keys, cstart, geo = build_grid(kps2, bounds)
    lists, dists = [None] * n1, [None] * n1
    for i1 in range(n1):
        if int(kps1["octave"][i1]) != 0:
            continue
        c = window(centres[i1, 0], centres[i1, 1], window_size, keys, cstart, geo, kps2)
        if c:
            lists[i1] = np.array(c, np.int64)
            dists[i1] = _POP[d1[i1][None, :] ^ d2[lists[i1]]].sum(1).astype(np.int64)

    # ---- phase B: the chain, in index order, over the precomputed distances
    m12 = np.full(n1, -1, np.int32)
    accepted = np.full(n1, -1, np.int64)       # the F2 feature a query was accepted with: never undone
    holder = np.full(n2, -1, np.int64)
    mdist = np.full(n2, INT_MAX, np.int64)
    for i1 in range(n1):
        if lists[i1] is None:
            continue
        c, d = lists[i1], dists[i1]
        live = mdist[c] > d
        st["skipped_taken"] += int((~live).sum())
        if not live.any():
            continue
        dl = d[live]
        k = int(np.argmin(dl))                 # the first minimum in list order
        best, best_idx = int(dl[k]), int(c[live][k])
        rest = np.delete(dl, k)
        second = int(rest.min()) if len(rest) else INT_MAX
        if best <= TH_LOW and F(best) < F(F(second) * F(nn_ratio)):
            if holder[best_idx] >= 0:
                m12[holder[best_idx]] = -1
                st["steals"] += 1
            st["single_candidate"] += second == INT_MAX
            m12[i1] = best_idx
            accepted[i1] = best_idx
            holder[best_idx] = i1
            mdist[best_idx] = best

    # ---- phase C: the histogram counts every acceptance; a query's bin is that of the feature it was accepted with
    if check_ori:
        bins = {i1: rot_bin(kps1["angle"][i1], kps2["angle"][accepted[i1]]) for i1 in range(n1) if accepted[i1] >= 0}
        sizes = [0] * 30
        for b in bins.values():
            if 0 <= b < 30:
                sizes[b] += 1
        ind = three_maxima(sizes)
        for i1, b in bins.items():
            if 0 <= b < 30 and b not in ind and m12[i1] >= 0:
                m12[i1] = -1
                st["removed"] += 1
    prev = None
    if prev_xy is not None:
        prev = centres.copy()
        for i1 in np.nonzero(m12 >= 0)[0]:
            prev[i1] = (kps2["x"][m12[i1]], kps2["y"][m12[i1]])
    if stats is not None:
        for k_, v in st.items():
            stats[k_] = stats.get(k_, 0) + int(v)
    return int((m12 >= 0).sum()), m12, prev


def three_maxima(sizes):
    """ComputeThreeMaxima (src/ORBmatcher.cc:2012-2053) -> (ind1, ind2, ind3)."""
    ind1 = ind2 = ind3 = -1
    max1 = max2 = max3 = 0
    for i, s in enumerate(sizes):
        if s > max1:
            max3, max2, max1, ind3, ind2, ind1 = max2, max1, s, ind2, ind1, i
        elif s > max2:
            max3, max2, ind3, ind2 = max2, s, ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if max2 < F(0.1) * F(max1):
        ind2 = ind3 = -1
    elif max3 < F(0.1) * F(max1):
        ind3 = -1
    return ind1, ind2, ind3


def invert(m12, n2: int):
    """matches21 of a final matches12 row."""
    m21 = np.full(n2, -1, np.int32)
    for i1 in np.nonzero(np.asarray(m12) >= 0)[0]:
        m21[m12[i1]] = i1
    return m21
