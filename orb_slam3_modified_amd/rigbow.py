"""The two-camera rig block of SearchByBoW over liborbx_rigbow.so (include/orbx_rigbow.h): the stacked rig frame (left features, then the
right ones at Nleft + j, as the reference's Frame holds them) from what FisheyeBatch left in HBM, and ORBmatcher::SearchByBoW
(src/ORBmatcher.cc:223-425 with F.Nleft != -1, :765-905 with NLeft != -1) for P pairs of stacked frames at once.  The stacked buffers are
what BowBatch.transform_device takes: the rig frame's FeatureVector is that call on them.  All arithmetic runs in the HIP kernels of the
library; this file only marshals buffers."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

from . import _lib
from ._lib import KP_DTYPE, OrbxRigBowRig, OrbxRigBowSide, addr, ptr
from ._pair import FV, PairResult, PairSide, count, host_call, new_results

FRAME, KEYFRAMES = 0, 1   # ORBX_RIGBOW_FRAME, ORBX_RIGBOW_KEYFRAMES
LDS_MAX = 152 * 1024


def lds_bytes(cap_a: int, cap_b: int) -> int:
    """The LDS block a pair of these capacities is staged in: B's descriptors, fv_feat list and match row, and the packed work list."""
    return 40 * int(cap_b) + 8 * min(int(cap_a), int(cap_b))


@dataclass
class StackedFrames:
    """orbx_rigbow_stack_device's outputs: kps [F, cap_s, 28] uint8 (keypoint records), desc [F, cap_s, 32] uint8, counts [F, 2] int32
    = {nl + nr, 0} ({-1, 0} for a malformed frame), nleft [F] int32 (-1 for a malformed frame)."""
    kps: object
    desc: object
    counts: object
    nleft: object
    nframes: int
    capacity: int


@dataclass
class RigBowSide(PairSide):
    """One side of the pairs (orbx_rigbow_side): MatchSide's fields on stacked frames and nleft [F] int32 (Nleft; -1 or None: single-camera
    frames).  Torch tensors or raw HBM addresses for bow_pairs_device, numpy arrays for bow_pairs."""
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
    nleft: object = None
    _STRUCT, _FIELDS = OrbxRigBowSide, ("kps", "desc", "counts") + FV + ("valid", "nleft")

    @classmethod
    def of(cls, stacked: StackedFrames, fv, valid=None) -> "RigBowSide":
        """From stack_device's result and a BowDeviceResult of the stacked buffers (or anything with fv_node / fv_ptr / fv_feat / fv_n)."""
        return cls(stacked.kps, stacked.desc, stacked.counts, fv.fv_node, fv.fv_ptr, fv.fv_feat, fv.fv_n, int(stacked.nframes),
                   int(stacked.capacity), valid, stacked.nleft)


@dataclass
class RigBowResult(PairResult):
    """nmatches [P] (the reference's return value, -1 for a malformed pair), b2a [P, b.capacity] (the A feature left in each B slot), a2b
    [P, a.capacity, 2] ({left B slot, right B slot} of each A feature); -1: none.  Torch tensors from bow_pairs_device, numpy arrays from
    bow_pairs.  result[p] = (nmatches, b2a row, a2b rows) of pair p on the host."""
    nmatches: object
    b2a: object
    a2b: object
    _ROWS = ("b2a", "a2b")


class RigBowBatch(_lib.SideHandle):
    """Stacked rig frames and their SearchByBoW for batches of frame pairs; one handle holds one stream and its scratch on one GPU."""

    lds_bytes = staticmethod(lds_bytes)

    def __init__(self, device_id: int = 0, library_path: Optional[str] = None):
        self._M = _lib.rigbow_lib(library_path) if library_path else _lib.rigbow_lib()
        self.device_id = int(device_id)
        super().__init__(self._M, "orbx_rigbow", int(device_id))

    def stack_device(self, kps_l, desc_l, counts_l, kps_r, desc_r, counts_r, cap_s: Optional[int] = None, stream=None,
                     out: Optional[StackedFrames] = None, nframes: Optional[int] = None, cap_l: Optional[int] = None,
                     cap_r: Optional[int] = None) -> StackedFrames:
        """orbx_rigbow_stack_device on the six buffers of FisheyeBatch.extract_device (torch tensors: desc [F, cap, 32]; or raw HBM addresses
        with nframes / cap_l / cap_r given); cap_s defaults to cap_l + cap_r.  Asynchronous on `stream` (None or 0: the handle's own).
        Without `out` the stacked tensors are allocated on desc_l's device (torch)."""
        F = int(desc_l.shape[0]) if nframes is None else int(nframes)
        cl = int(desc_l.shape[1]) if cap_l is None else int(cap_l)
        cr = int(desc_r.shape[1]) if cap_r is None else int(cap_r)
        cs = cl + cr if cap_s is None else int(cap_s)
        if out is None:
            import torch
            dev = desc_l.device if hasattr(desc_l, "device") else torch.device("cuda", self.device_id)
            out = StackedFrames(torch.empty((F, cs, KP_DTYPE.itemsize), dtype=torch.uint8, device=dev),
                                torch.empty((F, cs, 32), dtype=torch.uint8, device=dev), torch.empty((F, 2), dtype=torch.int32, device=dev),
                                torch.empty(F, dtype=torch.int32, device=dev), F, cs)
        rig = OrbxRigBowRig(*(addr(t) or None for t in (kps_l, desc_l, counts_l, kps_r, desc_r, counts_r)), F, cl, cr)
        self._check(self._M.orbx_rigbow_stack_device(self._h, C.byref(rig), cs, ptr(addr(out.kps)), ptr(addr(out.desc)), ptr(addr(out.counts)),
                                                     ptr(addr(out.nleft)), ptr(int(stream or 0))))
        return out

    def bow_pairs_device(self, a: RigBowSide, b: RigBowSide, pairs, mode: int = FRAME, nn_ratio: float = 0.7, check_orientation: bool = True,
                         stream=None, out: Optional[RigBowResult] = None, npairs: Optional[int] = None) -> RigBowResult:
        """orbx_rigbow_pairs_device: `pairs` [P, 2] int32 (frame of a, frame of b) on the device; asynchronous on `stream` (None or 0: the
        handle's own).  Without `out` the result tensors are allocated on the pairs' device (torch)."""
        P = count(pairs, npairs)
        if out is None:
            out = RigBowResult(*new_results(P, ((), (b.capacity,), (a.capacity, 2)), self, pairs))
        sa, sb = a._struct(), b._struct()
        self._check(self._M.orbx_rigbow_pairs_device(self._h, C.byref(sa), C.byref(sb), ptr(addr(pairs)), P, int(mode), float(nn_ratio),
                                                     int(bool(check_orientation)), ptr(addr(out.b2a)), ptr(addr(out.a2b)),
                                                     ptr(addr(out.nmatches)), ptr(int(stream or 0))))
        return out

    def bow_pairs(self, a: RigBowSide, b: RigBowSide, pairs, mode: int = FRAME, nn_ratio: float = 0.7, check_orientation: bool = True) -> RigBowResult:
        """orbx_rigbow_pairs on numpy arrays of the same layout; returns when the results are on the host."""
        ha, hb, pairs, P = host_call(a, b, pairs)
        out = RigBowResult(*new_results(P, ((), (hb.capacity,), (ha.capacity, 2))))
        sa, sb = ha._struct(), hb._struct()
        self._check(self._M.orbx_rigbow_pairs(self._h, C.byref(sa), C.byref(sb), ptr(pairs), P, int(mode), float(nn_ratio),
                                              int(bool(check_orientation)), ptr(out.b2a), ptr(out.a2b), ptr(out.nmatches)))
        return out
