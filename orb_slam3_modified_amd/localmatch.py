"""The batched SearchLocalPoints over liborbx_localmatch.so (include/orbx_localmatch.h): ORBmatcher::SearchByProjection(Frame&, map points)
(src/ORBmatcher.cc:43-141, Nleft == -1) for B (frame, local map) items at once on the keypoints and descriptors a batch extraction left in
HBM and the descriptor pool DistinctBatch fills.  All matching arithmetic runs in the HIP kernel of the library; this file only marshals
buffers.  The caller projects its map points (Frame::isInFrustum) and applies kp_match to its mvpMapPoints."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from ._window import LDS_MAX, MAX_CAPACITY, MAX_LEVELS, _table, _up16, lds_bytes  # noqa: F401  (re-exported)
from ._lib import KP_DTYPE, OrbxLocalMatchSide, addr, host_array as arr, host_view, ptr

POINT_DTYPE = np.dtype([("proj_x", "<f4"), ("proj_y", "<f4"), ("proj_xr", "<f4"), ("view_cos", "<f4"), ("level", "<i4"), ("obs", "<i4"),
                        ("point", "<i4"), ("in_view", "<i4")])
assert POINT_DTYPE.itemsize == 32


@dataclass
class LocalMatchSide:
    """The frame side (orbx_localmatch_side): kps [F, cap] keypoints (28 bytes each), desc [F, cap, 32], counts [F, 2], bounds [F, 4]
    float32 = {min_x, min_y, max_x, max_y}, uright [F, cap] float32 or None (monocular).  Torch tensors or raw HBM addresses for
    search_device, numpy arrays for search."""
    kps: object
    desc: object
    counts: object
    bounds: object
    nframes: int
    capacity: int
    uright: object = None

    def _struct(self) -> OrbxLocalMatchSide:
        return OrbxLocalMatchSide(*(addr(t) or None for t in (self.kps, self.desc, self.counts, self.uright, self.bounds)), int(self.nframes),
                                  int(self.capacity))

    def _host(self) -> "LocalMatchSide":
        """Contiguous numpy arrays of the ABI's element types."""
        K, cap = int(self.nframes), int(self.capacity)
        kps = np.ascontiguousarray(self.kps)
        assert kps.nbytes == K * cap * KP_DTYPE.itemsize
        return LocalMatchSide(kps, arr(self.desc, np.uint8, K, cap, 32), arr(self.counts, np.int32, K, 2), arr(self.bounds, np.float32, K, 4), K,
                              cap, None if self.uright is None else arr(self.uright, np.float32, K, cap))


@dataclass
class LocalMatchResult:
    """nmatches [B] (-1 for a malformed item), kp_match [B, cap] (the item's point bound to each keypoint, -1 untouched) and kp_obs [B, cap]
    (the rows after the call); torch tensors from search_device, numpy arrays from search.  result[b] = (nmatches, kp_match row, kp_obs row)
    of item b on the host."""
    nmatches: object
    kp_match: object
    kp_obs: object

    def __len__(self) -> int:
        return int(self.nmatches.shape[0])

    def __getitem__(self, b: int):
        return int(host_view(self.nmatches[b:b + 1])[0]), host_view(self.kp_match[b]), host_view(self.kp_obs[b])


class LocalMatchBatch(_lib.SideHandle):
    """Tracking's map-point matcher for batches of (frame, local map) items; one handle holds one stream and its scratch on one GPU."""

    def __init__(self, device_id: int = 0, library_path: Optional[str] = None):
        self._M = _lib.localmatch_lib(library_path) if library_path else _lib.localmatch_lib()
        self.device_id = int(device_id)
        super().__init__(self._M, "orbx_localmatch", int(device_id))

    def search_device(self, side: LocalMatchSide, frames, mp, nmp, pdesc, scale_factors, kp_obs, th: float = 1.0, nn_ratio: float = 0.8,
                      stream=None, out: Optional[LocalMatchResult] = None, nitems: Optional[int] = None, mcap: Optional[int] = None,
                      npoints: Optional[int] = None) -> LocalMatchResult:
        """orbx_localmatch_search_device: `frames` [B] int32, `mp` [B, mcap] records of POINT_DTYPE (a [B, mcap, 32] uint8 tensor), `nmp` [B]
        int32, `pdesc` [M, 32] uint8 and `kp_obs` [B, cap] int32 (updated in place) on the device, `scale_factors` a host array; asynchronous
        on `stream` (None or 0: the handle's own).  Without `out` kp_match and nmatches are allocated on the frames' device (torch); the
        result's kp_obs is the tensor passed in."""
        B = int(frames.shape[0]) if nitems is None else int(nitems)
        Q = int(mp.shape[1]) if mcap is None else int(mcap)
        M = int(pdesc.shape[0]) if npoints is None else int(npoints)
        if out is None:
            import torch
            dev = frames.device if hasattr(frames, "device") else torch.device("cuda", self.device_id)
            out = LocalMatchResult(torch.empty(B, dtype=torch.int32, device=dev),
                                   torch.empty((B, int(side.capacity)), dtype=torch.int32, device=dev), kp_obs)
        s = side._struct()
        _keep, pt, nl = _table(scale_factors)
        self._check(self._M.orbx_localmatch_search_device(self._h, C.byref(s), ptr(addr(frames)), B, ptr(addr(mp)), ptr(addr(nmp)), Q,
                                                          ptr(addr(pdesc)), M, pt, nl, float(th), float(nn_ratio), ptr(addr(kp_obs)),
                                                          ptr(addr(out.kp_match)), ptr(addr(out.nmatches)), ptr(int(stream or 0))))
        return out

    def search(self, side: LocalMatchSide, frames, mp, nmp, pdesc, scale_factors, kp_obs, th: float = 1.0,
               nn_ratio: float = 0.8) -> LocalMatchResult:
        """orbx_localmatch_search on numpy arrays of the same layout (`mp` [B, mcap] of POINT_DTYPE); returns when the results are on the
        host.  `kp_obs` is not changed: the updated rows are the result's."""
        hs = side._host()
        mp = np.ascontiguousarray(mp, POINT_DTYPE)
        B, Q = mp.shape
        frames, nmp = arr(frames, np.int32, B), arr(nmp, np.int32, B)
        pdesc = np.ascontiguousarray(pdesc, np.uint8).reshape(-1, 32)
        obs = arr(kp_obs, np.int32, B, hs.capacity).copy()
        out = LocalMatchResult(np.zeros(B, np.int32), np.zeros((B, hs.capacity), np.int32), obs)
        s = hs._struct()
        _keep, pt, nl = _table(scale_factors)
        self._check(self._M.orbx_localmatch_search(self._h, C.byref(s), ptr(frames), B, ptr(mp), ptr(nmp), Q, ptr(pdesc), len(pdesc), pt, nl,
                                                   float(th), float(nn_ratio), ptr(obs), ptr(out.kp_match), ptr(out.nmatches)))
        return out
