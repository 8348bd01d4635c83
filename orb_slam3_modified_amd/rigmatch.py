"""The two-camera rig blocks of Tracking's two projection matchers over liborbx_rigmatch.so (include/orbx_rigmatch.h): SearchLocalPoints
(src/ORBmatcher.cc:43-212) and SearchByProjection(CurrentFrame, LastFrame) (:1676-1886), both with Nleft != -1, for B items at once on the
left and right extractions and the left/right match tables FisheyeBatch left in HBM.  All matching arithmetic runs in the HIP kernel of the
library; this file only marshals buffers.  The caller projects its points into both cameras and applies kp_match to its stacked
mvpMapPoints: slot i < cap_l is left keypoint i, slot cap_l + j right keypoint j."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from ._window import LDS_MAX, MAX_CAPACITY, MAX_LEVELS, _table, rig_lds_bytes as lds_bytes  # noqa: F401  (re-exported)
from ._lib import KP_DTYPE, OrbxRigMatchSide, addr, host_array as arr, host_view, ptr

LOCAL_POINT_DTYPE = np.dtype([("proj_x", "<f4"), ("proj_y", "<f4"), ("view_cos", "<f4"), ("level", "<i4"), ("proj_xr", "<f4"), ("proj_yr", "<f4"),
                              ("view_cos_r", "<f4"), ("level_r", "<i4"), ("obs", "<i4"), ("point", "<i4"), ("in_view", "<i4"), ("in_view_r", "<i4")])
LAST_ITEM_DTYPE = np.dtype([("frame", "<i4"), ("direction", "<i4"), ("th", "<f4"), ("reserved", "<i4")])
LAST_POINT_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("u_r", "<f4"), ("v_r", "<f4"), ("angle", "<f4"), ("octave", "<i4"), ("obs", "<i4"),
                             ("point", "<i4"), ("valid", "<i4"), ("reserved", "<i4", (3,))])
assert LOCAL_POINT_DTYPE.itemsize == 48 and LAST_POINT_DTYPE.itemsize == 48 and LAST_ITEM_DTYPE.itemsize == 16


@dataclass
class RigSide:
    """The rig side (orbx_rigmatch_side): per camera kps [F, cap] raw keypoints (28 bytes each), desc [F, cap, 32], counts [F, 2]; l2r
    [F, cap_l] and r2l [F, cap_r] int32 (None for search_last_frame alone); bounds [F, 4] float32 = {min_x, min_y, max_x, max_y}, one row a
    frame for both grids.  Torch tensors or raw HBM addresses for the device forms, numpy arrays for the host forms."""
    kps_l: object
    desc_l: object
    counts_l: object
    kps_r: object
    desc_r: object
    counts_r: object
    l2r: object
    r2l: object
    bounds: object
    nframes: int
    cap_l: int
    cap_r: int

    @classmethod
    def from_fisheye(cls, kpsL, descL, countsL, kpsR, descR, countsR, stereo, bounds) -> "RigSide":
        """From what FisheyeBatch leaves: the six extraction buffers of extract / extract_device and the FisheyeStereo of finish /
        finish_device (its l2r and r2l), with the frames' bounds."""
        return cls(kpsL, descL, countsL, kpsR, descR, countsR, stereo.l2r, stereo.r2l, bounds, int(descL.shape[0]), int(descL.shape[1]),
                   int(descR.shape[1]))

    def _struct(self) -> OrbxRigMatchSide:
        return OrbxRigMatchSide(*(addr(t) or None for t in (self.kps_l, self.desc_l, self.counts_l, self.kps_r, self.desc_r, self.counts_r,
                                                            self.l2r, self.r2l, self.bounds)), int(self.nframes), int(self.cap_l), int(self.cap_r))

    def _host(self) -> "RigSide":
        """Contiguous numpy arrays of the ABI's element types."""
        K, cl, cr = int(self.nframes), int(self.cap_l), int(self.cap_r)
        kl, kr = np.ascontiguousarray(self.kps_l), np.ascontiguousarray(self.kps_r)
        assert kl.nbytes == K * cl * KP_DTYPE.itemsize and kr.nbytes == K * cr * KP_DTYPE.itemsize
        return RigSide(kl, arr(self.desc_l, np.uint8, K, cl, 32), arr(self.counts_l, np.int32, K, 2), kr, arr(self.desc_r, np.uint8, K, cr, 32),
                       arr(self.counts_r, np.int32, K, 2), None if self.l2r is None else arr(self.l2r, np.int32, K, cl),
                       None if self.r2l is None else arr(self.r2l, np.int32, K, cr), arr(self.bounds, np.float32, K, 4), K, cl, cr)


@dataclass
class RigMatchResult:
    """nmatches [B] (-1 for a malformed item), kp_match [B, cap_l + cap_r] (the item's point left in each slot, -1 untouched, -2 removed by
    the rotation filter) and kp_obs [B, cap_l + cap_r] (the rows after the call); torch tensors from the device forms, numpy arrays from
    the host forms.  result[b] = (nmatches, kp_match row, kp_obs row) of item b on the host."""
    nmatches: object
    kp_match: object
    kp_obs: object

    def __len__(self) -> int:
        return int(self.nmatches.shape[0])

    def __getitem__(self, b: int):
        return int(host_view(self.nmatches[b:b + 1])[0]), host_view(self.kp_match[b]), host_view(self.kp_obs[b])


class RigMatchBatch(_lib.SideHandle):
    """Tracking's two projection matchers on two-camera rig frames, for batches of items; one handle holds one stream and its scratch on
    one GPU."""

    LOCAL_POINT_DTYPE, LAST_ITEM_DTYPE, LAST_POINT_DTYPE = LOCAL_POINT_DTYPE, LAST_ITEM_DTYPE, LAST_POINT_DTYPE
    lds_bytes = staticmethod(lds_bytes)

    def __init__(self, device_id: int = 0, library_path: Optional[str] = None):
        self._M = _lib.rigmatch_lib(library_path) if library_path else _lib.rigmatch_lib()
        self.device_id = int(device_id)
        super().__init__(self._M, "orbx_rigmatch", int(device_id))

    def _out(self, side: RigSide, B: int, like, kp_obs, out):
        if out is not None:
            return out
        import torch
        dev = like.device if hasattr(like, "device") else torch.device("cuda", self.device_id)
        return RigMatchResult(torch.empty(B, dtype=torch.int32, device=dev),
                              torch.empty((B, int(side.cap_l) + int(side.cap_r)), dtype=torch.int32, device=dev), kp_obs)

    # ---- entry 1: SearchLocalPoints ----------------------------------------------------------------------
    def search_local_points_device(self, side: RigSide, frames, mp, nmp, pdesc, scale_factors, kp_obs, th: float = 1.0, nn_ratio: float = 0.8,
                                   stream=None, out: Optional[RigMatchResult] = None, nitems: Optional[int] = None,
                                   mcap: Optional[int] = None, npoints: Optional[int] = None) -> RigMatchResult:
        """orbx_rigmatch_local_device: `frames` [B] int32, `mp` [B, mcap] records of LOCAL_POINT_DTYPE (a [B, mcap, 48] uint8 tensor), `nmp`
        [B] int32, `pdesc` [M, 32] uint8 and `kp_obs` [B, cap_l + cap_r] int32 (updated in place) on the device, `scale_factors` a host
        array; asynchronous on `stream` (None or 0: the handle's own).  Without `out` kp_match and nmatches are allocated on the frames'
        device (torch); the result's kp_obs is the tensor passed in."""
        B = int(frames.shape[0]) if nitems is None else int(nitems)
        Q = int(mp.shape[1]) if mcap is None else int(mcap)
        M = int(pdesc.shape[0]) if npoints is None else int(npoints)
        out = self._out(side, B, frames, kp_obs, out)
        s = side._struct()
        _keep, pt, nl = _table(scale_factors)
        self._check(self._M.orbx_rigmatch_local_device(self._h, C.byref(s), ptr(addr(frames)), B, ptr(addr(mp)), ptr(addr(nmp)), Q,
                                                       ptr(addr(pdesc)), M, pt, nl, float(th), float(nn_ratio), ptr(addr(kp_obs)),
                                                       ptr(addr(out.kp_match)), ptr(addr(out.nmatches)), ptr(int(stream or 0))))
        return out

    def search_local_points(self, side: RigSide, frames, mp, nmp, pdesc, scale_factors, kp_obs, th: float = 1.0,
                            nn_ratio: float = 0.8) -> RigMatchResult:
        """orbx_rigmatch_local on numpy arrays of the same layout (`mp` [B, mcap] of LOCAL_POINT_DTYPE); returns when the results are on the
        host.  `kp_obs` is not changed: the updated rows are the result's."""
        hs = side._host()
        mp = np.ascontiguousarray(mp, LOCAL_POINT_DTYPE)
        B, Q = mp.shape
        slots = hs.cap_l + hs.cap_r
        frames, nmp = arr(frames, np.int32, B), arr(nmp, np.int32, B)
        pdesc = np.ascontiguousarray(pdesc, np.uint8).reshape(-1, 32)
        obs = arr(kp_obs, np.int32, B, slots).copy()
        out = RigMatchResult(np.zeros(B, np.int32), np.zeros((B, slots), np.int32), obs)
        s = hs._struct()
        _keep, pt, nl = _table(scale_factors)
        self._check(self._M.orbx_rigmatch_local(self._h, C.byref(s), ptr(frames), B, ptr(mp), ptr(nmp), Q, ptr(pdesc), len(pdesc), pt, nl,
                                                float(th), float(nn_ratio), ptr(obs), ptr(out.kp_match), ptr(out.nmatches)))
        return out

    # ---- entry 2: SearchByProjection(CurrentFrame, LastFrame) --------------------------------------------
    def search_last_frame_device(self, side: RigSide, items, points, nlast, pdesc, scale_factors, kp_obs, check_orientation: bool = True,
                                 stream=None, out: Optional[RigMatchResult] = None, nitems: Optional[int] = None,
                                 mcap: Optional[int] = None, npoints: Optional[int] = None) -> RigMatchResult:
        """orbx_rigmatch_last_device: `items` [B] records of LAST_ITEM_DTYPE (a [B, 16] uint8 tensor), `points` [B, mcap] records of
        LAST_POINT_DTYPE (a [B, mcap, 48] uint8 tensor), `nlast` [B] int32; the rest as search_local_points_device."""
        B = int(items.shape[0]) if nitems is None else int(nitems)
        Q = int(points.shape[1]) if mcap is None else int(mcap)
        M = int(pdesc.shape[0]) if npoints is None else int(npoints)
        out = self._out(side, B, items, kp_obs, out)
        s = side._struct()
        _keep, pt, nl = _table(scale_factors)
        self._check(self._M.orbx_rigmatch_last_device(self._h, C.byref(s), ptr(addr(items)), B, ptr(addr(points)), ptr(addr(nlast)), Q,
                                                      ptr(addr(pdesc)), M, pt, nl, int(bool(check_orientation)), ptr(addr(kp_obs)),
                                                      ptr(addr(out.kp_match)), ptr(addr(out.nmatches)), ptr(int(stream or 0))))
        return out

    def search_last_frame(self, side: RigSide, items, points, nlast, pdesc, scale_factors, kp_obs, check_orientation: bool = True) -> RigMatchResult:
        """orbx_rigmatch_last on numpy arrays of the same layout; returns when the results are on the host.  `kp_obs` is not changed."""
        hs = side._host()
        points = np.ascontiguousarray(points, LAST_POINT_DTYPE)
        B, Q = points.shape
        slots = hs.cap_l + hs.cap_r
        items = np.ascontiguousarray(items, LAST_ITEM_DTYPE).reshape(B)
        nlast = arr(nlast, np.int32, B)
        pdesc = np.ascontiguousarray(pdesc, np.uint8).reshape(-1, 32)
        obs = arr(kp_obs, np.int32, B, slots).copy()
        out = RigMatchResult(np.zeros(B, np.int32), np.zeros((B, slots), np.int32), obs)
        s = hs._struct()
        _keep, pt, nl = _table(scale_factors)
        self._check(self._M.orbx_rigmatch_last(self._h, C.byref(s), ptr(items), B, ptr(points), ptr(nlast), Q, ptr(pdesc), len(pdesc), pt, nl,
                                               int(bool(check_orientation)), ptr(obs), ptr(out.kp_match), ptr(out.nmatches)))
        return out
