"""The specification of the batched Fuse search (include/orbx_fuse.h) as the reference's loops, in numpy float32 / float64 scalars: one
operation at a time, no vectorised shortcut in the grid, the window or the gate.  Slow and plain on purpose."""
import math

import numpy as np

F = np.float32
COLS, ROWS = 64, 48
SENTINEL = (-1, 256)


def _round(v):
    """C's round() of a float32 value: halves away from zero."""
    v = float(v)
    return math.floor(v + 0.5) if v >= 0 else math.ceil(v - 0.5)


def cell_of(x, y, parm):
    """Frame::PosInGrid (src/Frame.cc:725-735) -> ix * 48 + iy, or -1 for a feature in no cell."""
    min_x, min_y, inv_w, inv_h = (F(v) for v in parm)
    with np.errstate(all="ignore"):
        px, py = F(F(F(x) - min_x) * inv_w), F(F(F(y) - min_y) * inv_h)
    if not (abs(float(px)) < 1e9 and abs(float(py)) < 1e9):
        return -1
    ix, iy = _round(px), _round(py)
    return -1 if ix < 0 or ix >= COLS or iy < 0 or iy >= ROWS else ix * ROWS + iy


def assign_grid(kps, parm):
    """mGrid flattened: 3072 lists of feature indices, each in ascending index (Frame::AssignFeaturesToGrid, src/Frame.cc:385-416)."""
    cells = [[] for _ in range(COLS * ROWS)]
    for i in range(len(kps)):
        c = cell_of(kps["x"][i], kps["y"][i], parm)
        if c >= 0:
            cells[c].append(i)
    return cells


def features_in_area(kps, cells, parm, x, y, r):
    """KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:704-748): the indices in the reference's order."""
    min_x, min_y, inv_w, inv_h = (F(v) for v in parm)
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
    for ix in range(n_min_x, n_max_x + 1):
        for iy in range(n_min_y, n_max_y + 1):
            for i in cells[ix * ROWS + iy]:
                distx, disty = F(F(kps["x"][i]) - x), F(F(kps["y"][i]) - y)
                if abs(distx) < r and abs(disty) < r:
                    out.append(i)
    return out


def passes_gate(kp_x, kp_y, kp_ur, octave, x, y, ur, inv_level_sigma2):
    """src/ORBmatcher.cc:1272-1296: float32 sums and products left to right, the comparison in double against the double literal."""
    ex, ey = F(F(x) - F(kp_x)), F(F(y) - F(kp_y))
    if F(kp_ur) >= 0:
        er = F(F(ur) - F(kp_ur))
        e2 = F(F(F(ex * ex) + F(ey * ey)) + F(er * er))
        return not float(F(e2 * F(inv_level_sigma2[octave]))) > 7.8
    e2 = F(F(ex * ex) + F(ey * ey))
    return not float(F(e2 * F(inv_level_sigma2[octave]))) > 5.99


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def nearest(kps, desc, uright, cells, parm, q, pdesc, inv_level_sigma2, gate, stats=None):
    """One query (a record of QUERY_DTYPE) -> (best_idx, best_dist)."""
    if q["point"] < 0:
        return SENTINEL
    qd = pdesc[q["point"]]
    best, bi = 256, -1
    for i in features_in_area(kps, cells, parm, q["x"], q["y"], q["r"]):
        octave = int(kps["octave"][i])
        if octave < q["min_level"] or octave > q["max_level"]:
            continue
        if gate and not passes_gate(kps["x"][i], kps["y"][i], -1.0 if uright is None else uright[i], octave, q["x"], q["y"], q["ur"],
                                    inv_level_sigma2):
            if stats is not None:
                stats["gated"] = stats.get("gated", 0) + 1
            continue
        d = hamming(qd, desc[i])
        if d < best:
            best, bi = d, i
        elif d == best and stats is not None:
            stats["ties"] = stats.get("ties", 0) + 1
    return bi, best


def search(kps, desc, counts, uright, gridparm, query, nquery, pairs, pdesc, inv_level_sigma2=None, gate=False, th_low=50, stats=None):
    """The whole call on host arrays of the ABI's layout -> (nfound [P], best_idx [P, qcap], best_dist [P, qcap]); a malformed pair gives -1
    and a sentinel row."""
    K, cap = kps.shape
    P, qcap = query.shape
    M = len(pdesc)
    nlevels = 0 if inv_level_sigma2 is None else len(inv_level_sigma2)
    nfound, bidx, bdist = np.zeros(P, np.int32), np.full((P, qcap), -1, np.int32), np.full((P, qcap), 256, np.int32)
    grids = {}
    for p in range(P):
        k, nq = int(pairs[p]), int(nquery[p])
        bad = not (0 <= k < K) or not (0 <= nq <= qcap)
        if not bad:
            n = int(counts[k, 0])
            bad = not (0 <= n <= cap) or any(int(query[p, q]["point"]) >= M for q in range(nq))
        if not bad:
            if k not in grids:
                grids[k] = assign_grid(kps[k, :n], gridparm[k])
            cells = grids[k]
            if gate:
                bad = any(not (0 <= int(kps[k, i]["octave"]) < nlevels) for c in cells for i in c)
        if bad:
            nfound[p] = -1
            continue
        ur = None if uright is None else uright[k, :n]
        for q in range(nq):
            bidx[p, q], bdist[p, q] = nearest(kps[k, :n], desc[k, :n], ur, cells, gridparm[k], query[p, q], pdesc, inv_level_sigma2, gate, stats)
        nfound[p] = int(((bidx[p] >= 0) & (bdist[p] <= th_low)).sum())
    return nfound, bidx, bdist
