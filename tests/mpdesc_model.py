"""The specification of the batched ComputeDistinctiveDescriptors (include/orbx_mpdesc.h) as the reference's loop
(src/MapPoint.cc:329-403), in numpy: the full N x N matrix, every row sorted, the element at int(0.5 * (N - 1)), a strict `<` scan from
INT_MAX.  Written the reference's way on purpose, not the kernels' (no selection without a sort, no packed key)."""
import numpy as np

MAX_OBS = 1024
INT_MAX = 2 ** 31 - 1
_POP = np.array([bin(v).count("1") for v in range(256)], np.uint8)


def distances(d):
    """:372-381 -- Distances[i][j] of the N descriptors d [N, 32]; the diagonal is 0."""
    return _POP[d[:, None, :] ^ d[None, :, :]].sum(2, dtype=np.int32)


def select_one(d, stats=None):
    """:369-397 for the descriptors a point's loop pushed -> (BestIdx, BestMedian)."""
    N = len(d)
    D = distances(d)
    best_median, best_idx = INT_MAX, 0
    medians = []
    for i in range(N):
        v = np.sort(D[i])
        median = int(v[int(0.5 * (N - 1))])
        medians.append(median)
        if median < best_median:
            best_median, best_idx = median, i
    if stats is not None:
        stats["tied"] = int(sum(1 for x in medians if x == best_median))
        stats["medians"] = medians
    return best_idx, best_median


def malformed(desc, counts, obs, obs_start, m, out_rows, table_rows):
    """What the header lists: obs_start not ascending or beyond nobs, N above the limit, an out row outside the table, a frame outside the
    side, a row outside 0 .. min(counts[frame][0], capacity) - 1."""
    K, cap = desc.shape[:2]
    s, e = int(obs_start[m]), int(obs_start[m + 1])
    if s < 0 or e < s or e > len(obs) or e - s > MAX_OBS:
        return True
    row = m if out_rows is None else int(out_rows[m])
    if not 0 <= row < table_rows:
        return True
    for o in obs[s:e]:
        f, r = int(o["frame"]), int(o["row"])
        if not 0 <= f < K or not 0 <= r < min(int(counts[f, 0]), cap):
            return True
    return False


def select(desc, counts, obs, obs_start, out_rows, table, stats=None):
    """The whole call on host arrays of the ABI's layout -> (best [M], median [M], the table with the winners' rows written; a copy)."""
    M = len(obs_start) - 1
    best, median, table = np.zeros(M, np.int32), np.zeros(M, np.int32), table.copy()
    for m in range(M):
        if malformed(desc, counts, obs, obs_start, m, out_rows, len(table)):
            best[m], median[m] = -2, -1
            continue
        o = obs[int(obs_start[m]):int(obs_start[m + 1])]
        if len(o) == 0:                                          # :365
            best[m], median[m] = -1, -1
            continue
        d = desc[o["frame"], o["row"]]
        st = None if stats is None else stats.setdefault(m, {})
        best[m], median[m] = select_one(d, st)
        table[m if out_rows is None else int(out_rows[m])] = d[best[m]]
    return best, median, table
