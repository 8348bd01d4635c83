"""The batched relocalization and Sim3 matchers over liborbx_projmatch.so (include/orbx_projmatch.h): ORBmatcher::SearchByProjection(
CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (src/ORBmatcher.cc:1889-2010, kind 0) and SearchByProjection(pKF, Scw, vpPoints[,
vpPointsKFs], vpMatched[, vpMatchedKF], th, ratioHamming) (:427-532, :534-646, kind 1) for B (frame, projected points) items at once on the
keypoints and descriptors a batch extraction left in HBM and the descriptor pool DistinctBatch fills.  All matching arithmetic runs in the
HIP kernel of the library; this file only marshals buffers.  The caller projects the points, folds every `continue` before
GetFeaturesInArea into `valid`, and applies kp_match to its mvpMapPoints / vpMatched (and vpMatchedKF)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from ._window import LDS_MAX, MAX_CAPACITY, MAX_LEVELS, _table, _up16, lds_bytes  # noqa: F401  (re-exported)
from ._lib import KP_DTYPE, OrbxProjMatchSide, addr, host_array as arr, host_view, ptr

KIND_RELOC, KIND_SIM3 = 0, 1
ITEM_DTYPE = np.dtype([("frame", "<i4"), ("kind", "<i4"), ("th", "<f4"), ("max_dist", "<f4")])
POINT_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("angle", "<f4"), ("level", "<i4"), ("point", "<i4"), ("valid", "<i4"), ("pad", "<i4", (2,))])
assert ITEM_DTYPE.itemsize == 16 and POINT_DTYPE.itemsize == 32


def max_dist_reloc(orb_dist: int) -> np.float32:
    """bestDist <= ORBdist (:1966) as the float limit of an item."""
    return np.float32(orb_dist)


def max_dist_sim3(ratio_hamming: float, th_low: int = 50) -> np.float32:
    """bestDist <= TH_LOW * ratioHamming (:523, :636): the float32 product."""
    return np.float32(np.float32(th_low) * np.float32(ratio_hamming))


@dataclass
class ProjMatchSide:
    """The frame side (orbx_projmatch_side): kps [F, cap] keypoints (28 bytes each), desc [F, cap, 32], counts [F, 2], bounds [F, 4]
    float32 = {min_x, min_y, max_x, max_y}.  Torch tensors or raw HBM addresses for search_device, numpy arrays for search."""
    kps: object
    desc: object
    counts: object
    bounds: object
    nframes: int
    capacity: int

    def _struct(self) -> OrbxProjMatchSide:
        return OrbxProjMatchSide(*(addr(t) or None for t in (self.kps, self.desc, self.counts, self.bounds)), int(self.nframes), int(self.capacity))

    def _host(self) -> "ProjMatchSide":
        """Contiguous numpy arrays of the ABI's element types."""
        K, cap = int(self.nframes), int(self.capacity)
        kps = np.ascontiguousarray(self.kps)
        assert kps.nbytes == K * cap * KP_DTYPE.itemsize
        return ProjMatchSide(kps, arr(self.desc, np.uint8, K, cap, 32), arr(self.counts, np.int32, K, 2), arr(self.bounds, np.float32, K, 4), K, cap)


@dataclass
class ProjMatchResult:
    """nmatches [B] (-1 for a malformed item) and kp_match [B, cap] (the item's point bound to each keypoint, -1 untouched, -2 bound and
    then set to NULL by the rotation filter); torch tensors from search_device, numpy arrays from search.
    result[b] = (nmatches, kp_match row) of item b on the host."""
    nmatches: object
    kp_match: object

    def __len__(self) -> int:
        return int(self.nmatches.shape[0])

    def __getitem__(self, b: int):
        return int(host_view(self.nmatches[b:b + 1])[0]), host_view(self.kp_match[b])


class ProjMatchBatch(_lib.SideHandle):
    """Relocalization's and LoopClosing's projection matchers for batches of (frame, projected points) items; one handle holds one stream
    and its scratch on one GPU."""

    def __init__(self, device_id: int = 0, library_path: Optional[str] = None):
        self._M = _lib.projmatch_lib(library_path) if library_path else _lib.projmatch_lib()
        self.device_id = int(device_id)
        super().__init__(self._M, "orbx_projmatch", int(device_id))

    def search_device(self, side: ProjMatchSide, items, points, npts, pdesc, scale_factors, kp_taken=None, check_orientation: bool = True,
                      stream=None, out: Optional[ProjMatchResult] = None, nitems: Optional[int] = None, mcap: Optional[int] = None,
                      npoints: Optional[int] = None) -> ProjMatchResult:
        """orbx_projmatch_search_device: `items` [B] records of ITEM_DTYPE (a [B, 16] uint8 tensor), `points` [B, mcap] records of
        POINT_DTYPE (a [B, mcap, 32] uint8 tensor), `npts` [B] int32, `pdesc` [M, 32] uint8 and `kp_taken` [B, cap] uint8 (or None: no
        keypoint holds a map point) on the device, `scale_factors` a host array; asynchronous on `stream` (None or 0: the handle's own).
        Without `out` kp_match and nmatches are allocated on the items' device (torch)."""
        B = int(items.shape[0]) if nitems is None else int(nitems)
        Q = int(points.shape[1]) if mcap is None else int(mcap)
        M = int(pdesc.shape[0]) if npoints is None else int(npoints)
        if out is None:
            import torch
            dev = items.device if hasattr(items, "device") else torch.device("cuda", self.device_id)
            out = ProjMatchResult(torch.empty(B, dtype=torch.int32, device=dev), torch.empty((B, int(side.capacity)), dtype=torch.int32, device=dev))
        s = side._struct()
        _keep, pt, nl = _table(scale_factors)
        self._check(self._M.orbx_projmatch_search_device(self._h, C.byref(s), ptr(addr(items)), B, ptr(addr(points)), ptr(addr(npts)), Q,
                                                         ptr(addr(pdesc)), M, pt, nl, int(bool(check_orientation)), ptr(addr(kp_taken)),
                                                         ptr(addr(out.kp_match)), ptr(addr(out.nmatches)), ptr(int(stream or 0))))
        return out

    def search(self, side: ProjMatchSide, items, points, npts, pdesc, scale_factors, kp_taken=None, check_orientation: bool = True) -> ProjMatchResult:
        """orbx_projmatch_search on numpy arrays of the same layout (`items` [B] of ITEM_DTYPE, `points` [B, mcap] of POINT_DTYPE,
        `kp_taken` [B, cap] uint8 or None); returns when the results are on the host.  `kp_taken` is not changed."""
        hs = side._host()
        points = np.ascontiguousarray(points, POINT_DTYPE)
        B, Q = points.shape
        items = np.ascontiguousarray(items, ITEM_DTYPE).reshape(B)
        npts = arr(npts, np.int32, B)
        pdesc = np.ascontiguousarray(pdesc, np.uint8).reshape(-1, 32)
        taken = None if kp_taken is None else arr(kp_taken, np.uint8, B, hs.capacity)
        out = ProjMatchResult(np.zeros(B, np.int32), np.zeros((B, hs.capacity), np.int32))
        s = hs._struct()
        _keep, pt, nl = _table(scale_factors)
        self._check(self._M.orbx_projmatch_search(self._h, C.byref(s), ptr(items), B, ptr(points), ptr(npts), Q, ptr(pdesc), len(pdesc), pt, nl,
                                                  int(bool(check_orientation)), ptr(taken), ptr(out.kp_match), ptr(out.nmatches)))
        return out
