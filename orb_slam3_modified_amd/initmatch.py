"""The batched SearchForInitialization over liborbx_initmatch.so (include/orbx_initmatch.h): ORBmatcher::SearchForInitialization
(src/ORBmatcher.cc:648-763) for P (frame, frame) pairs at once on the keypoints, descriptors and counts a batch extraction left in HBM.
All arithmetic runs in the HIP kernel of the library; this file only marshals buffers."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from ._lib import OrbxInitMatchSide, addr, ptr
from ._pair import PairResult, PairSide, count, host_call, new_results

LDS_MAX = 152 * 1024     # the largest LDS block of a workgroup (ORBX_INITMATCH_LDS lowers it)
MAX_CAPACITY = 32768


def lds_bytes(cap_a: int, cap_b: int) -> int:
    """What the LDS path needs for a pair of these capacities: its arrays (16-byte aligned) and room for one query's longest candidate list.
    A call takes the LDS path when this is within the handle's limit, the global-memory path otherwise."""
    p2 = 2
    while p2 < cap_b:
        p2 <<= 1
    parts = (32 * cap_a, 32 * cap_b, 4 * p2, 8 * cap_b, 2 * (64 * 48 + 1), 4 * (cap_a + 1), 4 * cap_b, 4 * cap_b, 4 * cap_a, 4 * cap_a)
    return sum((b + 15) & ~15 for b in parts) + 4 * cap_b


@dataclass
class InitSide(PairSide):
    """One side of the pairs (orbx_initmatch_side): kps [F, cap] keypoints (28 bytes each), desc [F, cap, 32], counts [F, 2].  Torch tensors
    or raw HBM addresses for pairs_device, numpy arrays for pairs."""
    kps: object
    desc: object
    counts: object
    nframes: int
    capacity: int
    _STRUCT, _FIELDS = OrbxInitMatchSide, ("kps", "desc", "counts")


@dataclass
class InitResult(PairResult):
    """nmatches [P] (the reference's return value, -1 for a malformed pair), matches12 [P, a.capacity], matches21 [P, b.capacity] or None
    (-1: no match), prev_xy [P, a.capacity, 2] or None (vbPrevMatched, updated); torch tensors from pairs_device, numpy arrays from pairs.
    result[p] = (nmatches, matches12 row, matches21 row) of pair p on the host."""
    nmatches: object
    matches12: object
    matches21: object
    prev_xy: object = None
    _ROWS = ("matches12", "matches21")


class InitMatchBatch(_lib.SideHandle):
    """Windowed frame-to-frame matches for batches of frame pairs; one handle holds one stream and its scratch on one GPU."""

    def __init__(self, device_id: int = 0, library=None):
        self._M = library or _lib.initmatch_lib()
        self.device_id = int(device_id)
        super().__init__(self._M, "orbx_initmatch", int(device_id))

    def pairs_device(self, a: InitSide, b: InitSide, pairs, bounds, window_size: int = 100, nn_ratio: float = 0.9, check_orientation: bool = True,
                     prev_xy=None, stream=None, out: Optional[InitResult] = None, npairs: Optional[int] = None) -> InitResult:
        """orbx_initmatch_pairs_device: `pairs` [P, 2] int32 (frame of a, frame of b) on the device, `bounds` (mnMinX, mnMinY, mnMaxX, mnMaxY)
        of b's frames, `prev_xy` [P, a.capacity, 2] float32 on the device (updated in place) or None; asynchronous on `stream` (None or 0: the
        handle's own).  Without `out` the result tensors are allocated on the pairs' device (torch)."""
        P = count(pairs, npairs)
        if out is None:
            out = InitResult(*new_results(P, ((), (a.capacity,), (b.capacity,)), self, pairs))
        out.prev_xy = prev_xy
        sa, sb = a._struct(), b._struct()
        bd = (C.c_float * 4)(*[float(v) for v in bounds])
        self._check(self._M.orbx_initmatch_pairs_device(self._h, C.byref(sa), C.byref(sb), ptr(addr(pairs)), P, bd, int(window_size),
                                                        float(nn_ratio), int(bool(check_orientation)), ptr(addr(prev_xy)),
                                                        ptr(addr(out.matches12)), ptr(addr(out.matches21)), ptr(addr(out.nmatches)),
                                                        ptr(int(stream or 0))))
        return out

    def pairs(self, a: InitSide, b: InitSide, pairs, bounds, window_size: int = 100, nn_ratio: float = 0.9, check_orientation: bool = True,
              prev_xy=None) -> InitResult:
        """orbx_initmatch_pairs on numpy arrays of the same layout; returns when the results are on the host.  `prev_xy` [P, a.capacity, 2]
        float32 is copied: the updated rows are the result's prev_xy."""
        ha, hb, pairs, P = host_call(a, b, pairs)
        prev = None if prev_xy is None else np.array(prev_xy, np.float32, order="C").reshape(P, ha.capacity, 2)
        out = InitResult(*new_results(P, ((), (ha.capacity,), (hb.capacity,))), prev)
        sa, sb = ha._struct(), hb._struct()
        bd = (C.c_float * 4)(*[float(v) for v in bounds])
        self._check(self._M.orbx_initmatch_pairs(self._h, C.byref(sa), C.byref(sb), ptr(pairs), P, bd, int(window_size), float(nn_ratio),
                                                 int(bool(check_orientation)), ptr(prev), ptr(out.matches12), ptr(out.matches21),
                                                 ptr(out.nmatches)))
        return out
