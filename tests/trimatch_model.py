"""The batched SearchForTriangulation's specification (include/orbx_trimatch.h) written as the reference's sequential loop
(src/ORBmatcher.cc:963-1133): per query a running bestDist that starts at 50 and a candidate that replaces on `dist <= bestDist`.  The gates
are evaluated in np.float32, one rounding per operation; the epipolar gate's last comparison is one of Python floats (doubles).

FeatureVectors are dicts node -> list of feature indices (the list order is the scan order).  `geom`: 12 float32 = F12 row-major, ep.x,
ep.y, pad."""
from __future__ import annotations

import numpy as np

from tests.match_batch_model import rotation_bin, three_maxima

TH_LOW = 50
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
_F = np.float32


def epipole_rejects(geom, x2, y2, scale) -> bool:
    """:1028-1033: the candidate lies too close to the epipole."""
    with np.errstate(all="ignore"):
        distex = _F(geom[9]) - _F(x2)
        distey = _F(geom[10]) - _F(y2)
        return bool(distex * distex + distey * distey < _F(100) * _F(scale))


def epipolar_passes(geom, x1, y1, x2, y2, unc) -> bool:
    """Pinhole::epipolarConstrain, src/CameraModels/Pinhole.cpp:115-128, F12(r, c) = geom[3 r + c]."""
    g = [_F(v) for v in geom[:9]]
    x1, y1, x2, y2 = _F(x1), _F(y1), _F(x2), _F(y2)
    with np.errstate(all="ignore"):
        a = x1 * g[0] + y1 * g[3] + g[6]
        b = x1 * g[1] + y1 * g[4] + g[7]
        c = x1 * g[2] + y1 * g[5] + g[8]
        num = a * x2 + b * y2 + c
        den = a * a + b * b
        if den == 0:
            return False
        dsqr = _F(num * num / den)
    return float(dsqr) < 3.84 * float(_F(unc))


def malformed(na, fv_a, nb, fv_b, kps_b, nlevels) -> bool:
    """What makes a pair of well-sized frames malformed: a listed feature that is not below its frame's count, or a listed B feature whose
    octave is outside [0, nlevels)."""
    if any(not 0 <= i < na for feats in fv_a.values() for i in feats):
        return True
    for feats in fv_b.values():
        for i in feats:
            if not 0 <= i < nb or not 0 <= int(kps_b["octave"][i]) < nlevels:
                return True
    return False


def _usable(has_point, uright, only_stereo, n):
    """(skip, stereo) per feature."""
    stereo = np.zeros(n, bool) if uright is None else np.asarray(uright, np.float32)[:n] >= 0
    skip = np.zeros(n, bool) if has_point is None else np.asarray(has_point)[:n] != 0
    if only_stereo:
        skip = skip | ~stereo
    return skip, stereo


def search_for_triangulation(kps_a, desc_a, fv_a, has_a, ur_a, kps_b, desc_b, fv_b, has_b, ur_b, geom, scale_factor, level_sigma2,
                             only_stereo=False, coarse=False, check_orientation=True, stats=None, restated=False):
    """(nmatches, matches12 [len(desc_a)]): matches12[i] = the B feature matched to A feature i, -1 for none; (-1, all -1) for a malformed
    pair.  `restated`: the winner as "argmin over all competing candidates, the last one on a tie" instead of the loop with its running
    bestDist.  `stats`, a dict, receives the counters the tests' vacuity guards read (see the module's tests)."""
    desc_a, desc_b = np.asarray(desc_a, np.uint8).reshape(-1, 32), np.asarray(desc_b, np.uint8).reshape(-1, 32)
    na, nb = len(desc_a), len(desc_b)
    m12 = np.full(na, -1, np.int32)
    if malformed(na, fv_a, nb, fv_b, kps_b, len(scale_factor)):
        return -1, m12
    geom = np.asarray(geom, np.float32)
    skip_a, stereo_a = _usable(has_a, ur_a, only_stereo, na)
    skip_b, stereo_b = _usable(has_b, ur_b, only_stereo, nb)
    st = dict(epipole_rejected=0, gate_rejected=0, gate_changed=0, ties_last=0, removed=0)
    bins = [[] for _ in range(30)]

    def gate(ia, ib, count):
        """Gates (2) and (3) for one candidate at dist <= 50."""
        x2, y2, o2 = kps_b["x"][ib], kps_b["y"][ib], int(kps_b["octave"][ib])
        if not stereo_a[ia] and not stereo_b[ib] and epipole_rejects(geom, x2, y2, scale_factor[o2]):
            st["epipole_rejected"] += count
            return False
        if coarse or epipolar_passes(geom, kps_a["x"][ia], kps_a["y"][ia], x2, y2, level_sigma2[o2]):
            return True
        st["gate_rejected"] += count
        return False

    for node in sorted(set(fv_a) & set(fv_b)):
        cand = np.asarray(fv_b[node], np.int64)
        if not len(cand):
            continue
        for ia in fv_a[node]:
            if skip_a[ia]:
                continue
            dist = _POP[desc_b[cand] ^ desc_a[ia]].sum(1)
            # every other candidate leaves the loop at `dist > TH_LOW` or at the skips before it without touching its state
            near = [int(j) for j in np.nonzero((dist <= TH_LOW) & ~skip_b[cand])[0]]
            best_idx = -1
            if not restated:
                best = TH_LOW
                for j in near:                                  # in list order
                    if dist[j] > best:
                        continue
                    if gate(ia, int(cand[j]), 1):
                        best_idx, best = int(cand[j]), int(dist[j])
            if restated or stats is not None:
                comp = [j for j in near if gate(ia, int(cand[j]), 0)]
                if comp:
                    dmin = min(int(dist[j]) for j in comp)
                    holders = [j for j in comp if dist[j] == dmin]
                    st["ties_last"] += len(holders) >= 2
                    if restated:
                        best_idx = int(cand[holders[-1]])
                if near:                                        # the winner were there no gates
                    dmin = min(int(dist[j]) for j in near)
                    ungated = int(cand[[j for j in near if dist[j] == dmin][-1]])
                    want = best_idx if not restated else (int(cand[holders[-1]]) if comp else -1)
                    st["gate_changed"] += ungated != want
            if best_idx >= 0:
                m12[ia] = best_idx
                if check_orientation:
                    b = rotation_bin(kps_a["angle"][ia], kps_b["angle"][best_idx])
                    if 0 <= b < 30:
                        bins[b].append(ia)
    if check_orientation:
        keep = three_maxima([len(b) for b in bins])
        for i, members in enumerate(bins):
            if i not in keep:
                for ia in members:
                    m12[ia] = -1
                    st["removed"] += 1
    if stats is not None:
        stats.update(st)
    return int((m12 >= 0).sum()), m12


def matched_pairs(m12):
    """vMatchedPairs of a matches12 row."""
    return [(int(i), int(m12[i])) for i in np.nonzero(np.asarray(m12) >= 0)[0]]
