"""A plain numpy restatement of Frame::ComputeStereoMatches (src/Frame.cc:811-981) in the reference's own order: the row lists of the right
keypoints, per left keypoint the candidate loop in ascending right index (first minimum), the 11 x 11 SAD over 11 shifts on the left
keypoint's level, the parabola, the disparity gate with its 0.01 branch, then the sort and the removal of the tail above
1.5f * 1.4f * median.  Every float step is np.float32; `uL - 0.01` is taken in double and then cast.  Shares no code with the kernels'
Python wrappers: the tests hold it to oracle.pyoracle.stereo_matches byte for byte, then ask it which branch decided each keypoint.

compute_stereo_matches(...) -> (u_right, depth, kept, stats).  stats holds the counters of COUNTERS and, per left keypoint,
stats["branch"][i] (one of BRANCHES: the branch that decided it) and stats["rec"][i] (what it saw on the way)."""
import math

import numpy as np

F32 = np.float32
TH_HIGH, TH_LOW = 100, 50
BRANCHES = ("empty_row", "maxu_negative", "no_candidate", "hamming", "border", "shift_first", "shift_last", "delta", "disparity_negative",
            "disparity_max", "accepted", "accepted_001", "median_removed")
COUNTERS = ("gate_row", "gate_level_below", "gate_level_above", "gate_u_below", "gate_u_above", "gate_pass", "hamming_tie", "hamming_over_high",
            "hamming_75_to_99", "hamming_74", "band_clamped", "band_on_max", "band_on_min", "sad_tie", "delta_zero", "delta_nonzero",
            "median_even", "median_odd", "median_tie", "median_zero", "removed") + BRANCHES


def _round(x):
    """std::round of a float: halves away from zero."""
    x = float(x)
    return F32(math.copysign(math.floor(abs(x) + 0.5), x))


def _hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def row_band(y, octave, scale):
    r = F32(2.0) * F32(scale[octave])
    return int(math.floor(F32(y) - r)), int(math.ceil(F32(y) + r))


def compute_stereo_matches(kpsL, descL, kpsR, descR, pyrL, pyrR, scale, inv_scale, mb, mbf):
    scale, inv_scale = np.asarray(scale, F32), np.asarray(inv_scale, F32)
    mb, mbf = F32(mb), F32(mbf)
    N, Nr = len(kpsL), len(kpsR)
    u_right, depth = np.full(N, -1.0, F32), np.full(N, -1.0, F32)
    st = {k: 0 for k in COUNTERS}
    st["branch"], st["rec"] = [None] * N, [dict() for _ in range(N)]
    n_rows = pyrL[0].shape[0]
    rows = [[] for _ in range(n_rows)]
    for iR in range(Nr):
        minr, maxr = row_band(kpsR[iR]["y"], int(kpsR[iR]["octave"]), scale)
        st["band_clamped"] += minr < -1 or maxr >= n_rows
        for yi in range(minr, maxr + 1):
            if 0 <= yi < n_rows:
                rows[yi].append(iR)
    minD, maxD = F32(0.0), mbf / mb
    th_orb = (TH_HIGH + TH_LOW) // 2
    dist_idx = []
    for iL in range(N):
        kp, rec = kpsL[iL], st["rec"][iL]
        level, vL, uL = int(kp["octave"]), F32(kp["y"]), F32(kp["x"])

        def decide(branch):
            st["branch"][iL] = branch
            st[branch] += 1

        cand = rows[int(vL)]
        st["gate_row"] += Nr - len(cand)
        if not cand:
            decide("empty_row")
            continue
        minU, maxU = uL - maxD, uL - minD
        if maxU < 0:
            decide("maxu_negative")
            continue
        best, best_idx, passed = TH_HIGH, 0, 0
        for iR in cand:
            o, uR = int(kpsR[iR]["octave"]), F32(kpsR[iR]["x"])
            minr, maxr = row_band(kpsR[iR]["y"], o, scale)
            st["band_on_max"] += maxr == int(vL)
            st["band_on_min"] += minr == int(vL)
            if o < level - 1 or o > level + 1:
                st["gate_level_below" if o < level - 1 else "gate_level_above"] += 1
                continue
            if not (uR >= minU and uR <= maxU):
                st["gate_u_below" if uR < minU else "gate_u_above"] += 1
                continue
            passed += 1
            d = _hamming(descL[iL], descR[iR])
            st["hamming_tie"] += d == best and d < TH_HIGH
            st["hamming_over_high"] += d >= TH_HIGH
            if d < best:
                best, best_idx = d, iR
        st["gate_pass"] += passed
        rec.update(passed=passed, best_dist=best, best_idx=best_idx if best < TH_HIGH else -1)
        if not best < th_orb:
            st["hamming_75_to_99"] += th_orb <= best < TH_HIGH
            decide("hamming" if passed else "no_candidate")
            continue
        st["hamming_74"] += best == th_orb - 1
        uR0 = F32(kpsR[best_idx]["x"])
        sf = inv_scale[level]
        su_l, sv_l, su_r = _round(uL * sf), _round(vL * sf), _round(uR0 * sf)
        w, L = 5, 5
        IL, IR = pyrL[level], pyrR[level]
        iniu, endu = su_r + F32(L) - F32(w), su_r + F32(L) + F32(w) + F32(1)
        rec.update(scaled_uR0=float(su_r), endu=float(endu))
        if iniu < 0 or endu >= IL.shape[1]:
            decide("border")
            continue
        r0, c0 = int(sv_l - F32(w)), int(su_l - F32(w))
        a = IL[r0:r0 + 2 * w + 1, c0:c0 + 2 * w + 1].astype(np.int64)
        assert a.shape == (11, 11), "left window outside the plane: the input left the domain"
        best_s, best_inc, dists = None, 0, []
        for inc in range(-L, L + 1):
            cr = int(su_r + F32(inc) - F32(w))
            b = IR[r0:r0 + 2 * w + 1, cr:cr + 2 * w + 1].astype(np.int64)
            assert cr >= 0 and b.shape == (11, 11), "right window outside the plane"
            dist = F32(np.abs(a - b).sum())
            if best_s is None or dist < F32(best_s):
                best_s, best_inc = int(dist), inc
            dists.append(dist)
        st["sad_tie"] += sum(1 for d in dists if d == F32(best_s)) > 1
        rec.update(inc=best_inc, sad=best_s, sads=[int(d) for d in dists])
        if best_inc == -L or best_inc == L:
            decide("shift_first" if best_inc == -L else "shift_last")
            continue
        d1, d2, d3 = dists[L + best_inc - 1], dists[L + best_inc], dists[L + best_inc + 1]
        delta = (d1 - d3) / (F32(2.0) * (d1 + d3 - F32(2.0) * d2))
        rec["delta"] = float(delta)
        if delta < -1 or delta > 1:
            decide("delta")
            continue
        st["delta_zero" if delta == 0 else "delta_nonzero"] += 1
        best_u = scale[level] * (su_r + F32(best_inc) + delta)
        disparity = uL - best_u
        rec["disparity"] = float(disparity)
        if disparity >= minD and disparity < maxD:
            small = disparity <= 0
            if small:
                disparity = F32(0.01)
                best_u = F32(float(uL) - 0.01)
            depth[iL], u_right[iL] = mbf / disparity, best_u
            dist_idx.append((best_s, iL))
            decide("accepted_001" if small else "accepted")
        else:
            decide("disparity_negative" if disparity < minD else "disparity_max")
    if not dist_idx:
        return u_right, depth, 0, st
    dist_idx.sort()
    n = len(dist_idx)
    median = F32(dist_idx[n // 2][0])
    th = F32(F32(1.5) * F32(1.4)) * median
    st["median_even" if n % 2 == 0 else "median_odd"] += 1
    st["median_tie"] += sum(1 for s, _ in dist_idx if s == dist_idx[n // 2][0]) > 1
    st["median_zero"] += median == 0
    rec_f = dict(n=n, median=int(median), th=float(th), sads=[s for s, _ in dist_idx])
    kept = n
    for s, i in reversed(dist_idx):
        if F32(s) < th:
            break
        u_right[i], depth[i] = F32(-1), F32(-1)
        st[st["branch"][i]] -= 1
        st["branch"][i] = "median_removed"
        st["median_removed"] += 1
        st["removed"] += 1
        kept -= 1
    st["filter"] = rec_f
    return u_right, depth, kept, st
