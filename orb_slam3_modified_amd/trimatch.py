"""The batched SearchForTriangulation over liborbx_trimatch.so (include/orbx_trimatch.h): ORBmatcher::SearchForTriangulation
(src/ORBmatcher.cc:907-1146, single camera, pinhole) for P (keyframe, keyframe) pairs at once on the descriptors, keypoints and
FeatureVectors a batch extraction and BowBatch.transform_device left in HBM.  All matching arithmetic runs in the HIP kernel of the library;
this file only marshals buffers.  The caller computes each pair's F12 and epipole (`fundamental` is a convenience for Python callers)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from ._lib import OrbxTriMatchSide, addr, ptr
from ._pair import FV, PairResult, PairSide, count, host_call, new_results

LDS_MAX = 152 * 1024     # the largest LDS block of a workgroup (ORBX_TRIMATCH_LDS lowers it)
MAX_CAPACITY = 65536
MAX_LEVELS = 16


def lds_bytes(cap_a: int, cap_b: int) -> int:
    """What the LDS path needs for a pair of these capacities.  A call takes the LDS path when this is within the handle's limit, the
    global-memory path otherwise."""
    return 32 * (cap_a + cap_b) + 16 * (min(cap_a, cap_b) + cap_a // 16 + 1) + 4 * (2 * cap_a + cap_b)


def fundamental(K1, R12, t12, K2) -> np.ndarray:
    """F12 = K1^-T [t12]x R12 K2^-1 (src/CameraModels/Pinhole.cpp:109-112) as 9 float32 values, row-major.

    A convenience for Python callers: computed in float64 with numpy and rounded once, so it is NOT pinned to Eigen's float32 rounding of the
    same product.  A caller that must reproduce the reference's matches bit for bit passes the F12 its own Eigen computes."""
    K1, R12, K2 = (np.asarray(m, np.float64).reshape(3, 3) for m in (K1, R12, K2))
    t = np.asarray(t12, np.float64).reshape(3)
    tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    return (np.linalg.inv(K1.T) @ tx @ R12 @ np.linalg.inv(K2)).astype(np.float32).reshape(9)


def geometry(F12, ep) -> np.ndarray:
    """One pair's row of `geom`: F12 row-major, ep.x, ep.y, one pad value."""
    g = np.zeros(12, np.float32)
    g[:9] = np.asarray(F12, np.float32).reshape(9)
    g[9:11] = np.asarray(ep, np.float32).reshape(2)
    return g


@dataclass
class TriMatchSide(PairSide):
    """One side of the pairs (orbx_trimatch_side): kps [F, cap] keypoints (28 bytes each), desc [F, cap, 32], counts [F, 2], the four
    FeatureVector arrays as BowDeviceResult holds them, has_point [F, cap] uint8 or None (no feature has a MapPoint), uright [F, cap] float32
    or None (monocular).  Torch tensors or raw HBM addresses for pairs_device, numpy arrays for pairs."""
    kps: object
    desc: object
    counts: object
    fv_node: object
    fv_ptr: object
    fv_feat: object
    fv_n: object
    nframes: int
    capacity: int
    has_point: object = None
    uright: object = None
    _STRUCT, _FIELDS = OrbxTriMatchSide, ("kps", "desc", "counts") + FV + ("has_point", "uright")

    @classmethod
    def of(cls, kps, desc, counts, fv, nframes: int, capacity: int, has_point=None, uright=None) -> "TriMatchSide":
        """From a batch extraction's buffers and a BowDeviceResult (or anything with fv_node / fv_ptr / fv_feat / fv_n)."""
        return cls(kps, desc, counts, fv.fv_node, fv.fv_ptr, fv.fv_feat, fv.fv_n, int(nframes), int(capacity), has_point, uright)


@dataclass
class TriMatchResult(PairResult):
    """nmatches [P] (the reference's return value, -1 for a malformed pair), matches12 [P, a.capacity] (vMatches12; -1: no match); torch
    tensors from pairs_device, numpy arrays from pairs.  result[p] = (nmatches, matches12 row) of pair p on the host."""
    nmatches: object
    matches12: object
    _ROWS = ("matches12",)

    def matched_pairs(self, p: int) -> list:
        """vMatchedPairs of pair p: (index in A, index in B), ascending in the A index."""
        row = self[p][1]
        return [(int(i), int(row[i])) for i in np.nonzero(row >= 0)[0]]


def _tables(scale_factor, level_sigma2):
    s, q = np.ascontiguousarray(scale_factor, np.float32).ravel(), np.ascontiguousarray(level_sigma2, np.float32).ravel()
    if len(s) != len(q):
        raise ValueError("scale_factor and level_sigma2 differ in length")
    fp = C.POINTER(C.c_float)
    return s, q, s.ctypes.data_as(fp), q.ctypes.data_as(fp), len(s)


class TriMatchBatch(_lib.SideHandle):
    """Epipolar-gated matches for batches of keyframe pairs; one handle holds one stream and its scratch on one GPU."""

    def __init__(self, device_id: int = 0):
        self._M = _lib.trimatch_lib()
        self.device_id = int(device_id)
        super().__init__(self._M, "orbx_trimatch", int(device_id))

    def pairs_device(self, a: TriMatchSide, b: TriMatchSide, pairs, geom, scale_factor, level_sigma2, only_stereo: bool = False,
                     coarse: bool = False, check_orientation: bool = True, stream=None, out: Optional[TriMatchResult] = None,
                     npairs: Optional[int] = None) -> TriMatchResult:
        """orbx_trimatch_pairs_device: `pairs` [P, 2] int32 (keyframe of a, keyframe of b) and `geom` [P, 12] float32 on the device,
        `scale_factor` / `level_sigma2` host arrays of b's extractor; asynchronous on `stream` (None or 0: the handle's own).  Without `out`
        the result tensors are allocated on the pairs' device (torch)."""
        P = count(pairs, npairs)
        if out is None:
            out = TriMatchResult(*new_results(P, ((), (a.capacity,)), self, pairs))
        sa, sb = a._struct(), b._struct()
        _s, _q, ps, pq, nl = _tables(scale_factor, level_sigma2)
        self._check(self._M.orbx_trimatch_pairs_device(self._h, C.byref(sa), C.byref(sb), ptr(addr(pairs)), P, ptr(addr(geom)), ps, pq, nl,
                                                       int(bool(only_stereo)), int(bool(coarse)), int(bool(check_orientation)),
                                                       ptr(addr(out.matches12)), ptr(addr(out.nmatches)), ptr(int(stream or 0))))
        return out

    def pairs(self, a: TriMatchSide, b: TriMatchSide, pairs, geom, scale_factor, level_sigma2, only_stereo: bool = False, coarse: bool = False,
              check_orientation: bool = True) -> TriMatchResult:
        """orbx_trimatch_pairs on numpy arrays of the same layout; returns when the results are on the host."""
        ha, hb, pairs, P = host_call(a, b, pairs)
        geom = np.ascontiguousarray(geom, np.float32).reshape(P, 12)
        out = TriMatchResult(*new_results(P, ((), (ha.capacity,))))
        sa, sb = ha._struct(), hb._struct()
        _s, _q, ps, pq, nl = _tables(scale_factor, level_sigma2)
        self._check(self._M.orbx_trimatch_pairs(self._h, C.byref(sa), C.byref(sb), ptr(pairs), P, ptr(geom), ps, pq, nl, int(bool(only_stereo)),
                                                int(bool(coarse)), int(bool(check_orientation)), ptr(out.matches12), ptr(out.nmatches)))
        return out
