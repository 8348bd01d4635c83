"""The batched SearchByBoW over liborbx_match.so (include/orbx_match.h): ORBmatcher::SearchByBoW (src/ORBmatcher.cc:223-425, :765-905) for P
(frame, frame) pairs at once on the descriptors, keypoints and FeatureVectors a batch extraction and BowBatch.transform_device left in HBM.
All arithmetic runs in the HIP kernel of the library; this file only marshals buffers."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

from . import _lib
from ._lib import OrbxMatchSide, addr, ptr
from ._pair import FV, PairResult, PairSide, count, host_call, new_results

FRAME, KEYFRAMES = 0, 1   # ORBX_MATCH_FRAME, ORBX_MATCH_KEYFRAMES


@dataclass
class MatchSide(PairSide):
    """One side of the pairs (orbx_match_side): kps [F, cap] keypoints (28 bytes each), desc [F, cap, 32], counts [F, 2], the four
    FeatureVector arrays as BowDeviceResult holds them, valid [F, cap] uint8 or None.  Torch tensors or raw HBM addresses for
    bow_pairs_device, numpy arrays for bow_pairs."""
    kps: object
    desc: object
    counts: object
    fv_node: object
    fv_ptr: object
    fv_feat: object
    fv_n: object
    nframes: int
    capacity: int
    valid: object = None
    _STRUCT, _FIELDS = OrbxMatchSide, ("kps", "desc", "counts") + FV + ("valid",)

    @classmethod
    def of(cls, kps, desc, counts, fv, nframes: int, capacity: int, valid=None) -> "MatchSide":
        """From a batch extraction's buffers and a BowDeviceResult (or anything with fv_node / fv_ptr / fv_feat / fv_n)."""
        return cls(kps, desc, counts, fv.fv_node, fv.fv_ptr, fv.fv_feat, fv.fv_n, int(nframes), int(capacity), valid)


@dataclass
class MatchResult(PairResult):
    """nmatches [P] (the reference's return value, -1 for a malformed pair), b2a [P, b.capacity], a2b [P, a.capacity] (-1: no match); torch
    tensors from bow_pairs_device, numpy arrays from bow_pairs.  result[p] = (nmatches, b2a row, a2b row) of pair p on the host."""
    nmatches: object
    b2a: object
    a2b: object
    _ROWS = ("b2a", "a2b")


class MatchBatch(_lib.SideHandle):
    """Putative matches for batches of frame pairs; one handle holds one stream and its scratch on one GPU."""

    def __init__(self, device_id: int = 0):
        self._M = _lib.match_lib()
        self.device_id = int(device_id)
        super().__init__(self._M, "orbx_match", int(device_id))

    def bow_pairs_device(self, a: MatchSide, b: MatchSide, pairs, mode: int = FRAME, nn_ratio: float = 0.7, check_orientation: bool = True,
                         stream=None, out: Optional[MatchResult] = None, npairs: Optional[int] = None) -> MatchResult:
        """orbx_match_bow_pairs_device: `pairs` [P, 2] int32 (frame of a, frame of b) on the device; asynchronous on `stream` (None or 0: the
        handle's own).  Without `out` the result tensors are allocated on the pairs' device (torch)."""
        P = count(pairs, npairs)
        if out is None:
            out = MatchResult(*new_results(P, ((), (b.capacity,), (a.capacity,)), self, pairs))
        sa, sb = a._struct(), b._struct()
        self._check(self._M.orbx_match_bow_pairs_device(self._h, C.byref(sa), C.byref(sb), ptr(addr(pairs)), P, int(mode), float(nn_ratio),
                                                        int(bool(check_orientation)), ptr(addr(out.b2a)), ptr(addr(out.a2b)),
                                                        ptr(addr(out.nmatches)), ptr(int(stream or 0))))
        return out

    def bow_pairs(self, a: MatchSide, b: MatchSide, pairs, mode: int = FRAME, nn_ratio: float = 0.7, check_orientation: bool = True) -> MatchResult:
        """orbx_match_bow_pairs on numpy arrays of the same layout; returns when the results are on the host."""
        ha, hb, pairs, P = host_call(a, b, pairs)
        out = MatchResult(*new_results(P, ((), (hb.capacity,), (ha.capacity,))))
        sa, sb = ha._struct(), hb._struct()
        self._check(self._M.orbx_match_bow_pairs(self._h, C.byref(sa), C.byref(sb), ptr(pairs), P, int(mode), float(nn_ratio),
                                                 int(bool(check_orientation)), ptr(out.b2a), ptr(out.a2b), ptr(out.nmatches)))
        return out
