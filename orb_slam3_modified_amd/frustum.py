"""The batched Frame::isInFrustum over liborbx_frustum.so (include/orbx_frustum.h): src/Frame.cc:512-574 (Nleft == -1, pinhole) with
MapPoint::PredictScale for B (pose, local map) items at once over a table of map points that stays in HBM.  The rows it writes are the
orbx_localmatch_point records LocalMatchBatch.search_device reads, so `project(...).mp` goes into the search as it is.  All projection
arithmetic runs in the HIP kernel of the library (or, for `reference`, in its plain C++ host twin); this file only marshals buffers."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from ._lib import OrbxError, addr, host_array as arr, host_view, ptr
from .localmatch import POINT_DTYPE

MAX_LEVELS = 16
SUM_LTR, SUM_TREE = 0, 1
LOG_DOUBLE, LOG_FLOAT = 0, 1
TABLE_DTYPE = np.dtype([("pos", "<f4", 3), ("min_inv", "<f4"), ("normal", "<f4", 3), ("max_inv", "<f4"), ("max_dist", "<f4"), ("pad", "<f4", 3)])
ITEM_DTYPE = np.dtype([("Rcw", "<f4", 9), ("tcw", "<f4", 3), ("Ow", "<f4", 3), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"),
                       ("mbf", "<f4"), ("bounds", "<f4", 4), ("far_th", "<f4"), ("pad", "<f4", 3)])
assert TABLE_DTYPE.itemsize == 48 and ITEM_DTYPE.itemsize == 112


@dataclass
class FrustumResult:
    """mp [B, mcap] records of POINT_DTYPE (from `project`: a [B, mcap, 32] uint8 torch tensor on the device), depth [B, mcap] float32 or
    None, ntomatch [B] int32 (-1 for a malformed item)."""
    mp: object
    depth: object
    ntomatch: object

    def host(self) -> "FrustumResult":
        """The same on the host: mp as a [B, mcap] array of POINT_DTYPE."""
        mp = host_view(self.mp)
        if mp.dtype != POINT_DTYPE:
            mp = np.ascontiguousarray(mp).view(POINT_DTYPE).reshape(mp.shape[0], mp.shape[1])
        return FrustumResult(mp, host_view(self.depth), host_view(self.ntomatch))


def level_thresholds(log_scale_factor: float, nlevels: int, log_kind: int = LOG_DOUBLE) -> np.ndarray:
    """orbx_frustum_level_thresholds: T[n], n in 0 .. nlevels-2, the largest float whose predicted level is <= n.  Host only."""
    M = _lib.frustum_lib()
    T = np.zeros(max(int(nlevels) - 1, 0), np.float32)
    rc = M.orbx_frustum_level_thresholds(float(log_scale_factor), int(nlevels), int(log_kind), ptr(T) if len(T) else None)
    if rc < 0:
        raise OrbxError(rc, (M.orbx_frustum_last_error(None) or b"").decode())
    return T


def _host_call(points, obs, items, idx, nmp):
    points = np.ascontiguousarray(points, TABLE_DTYPE).ravel()
    items = np.ascontiguousarray(items, ITEM_DTYPE).ravel()
    idx = np.ascontiguousarray(idx, np.int32)
    B, Q = idx.shape
    assert len(items) == B
    return points, arr(obs, np.int32, len(points)), items, idx, arr(nmp, np.int32, B), B, Q


def reference(points, obs, items, idx, nmp, log_scale_factor: float, nlevels: int, cos_limit: float = 0.5, sum_order: int = SUM_LTR,
              log_kind: int = LOG_DOUBLE, want_depth: bool = True) -> FrustumResult:
    """orbx_frustum_project_reference: the host twin on numpy arrays (libm's log for every point, no thresholds, no device)."""
    M = _lib.frustum_lib()
    points, obs, items, idx, nmp, B, Q = _host_call(points, obs, items, idx, nmp)
    out = FrustumResult(np.zeros((B, Q), POINT_DTYPE), np.zeros((B, Q), np.float32) if want_depth else None, np.zeros(B, np.int32))
    rc = M.orbx_frustum_project_reference(ptr(points), ptr(obs), len(points), ptr(items), B, ptr(idx), ptr(nmp), Q, float(log_scale_factor),
                                          int(nlevels), float(cos_limit), int(sum_order), int(log_kind), ptr(out.mp), ptr(out.depth),
                                          ptr(out.ntomatch))
    if rc < 0:
        raise OrbxError(rc, (M.orbx_frustum_last_error(None) or b"").decode())
    return out


class FrustumBatch(_lib.SideHandle):
    """Tracking's frustum test for batches of (pose, local map) items; one handle holds one stream and the thresholds of its last
    (log_scale_factor, nlevels, log_kind) on one GPU."""

    def __init__(self, device_id: int = 0, library_path: Optional[str] = None):
        self._M = _lib.frustum_lib(library_path) if library_path else _lib.frustum_lib()
        self.device_id = int(device_id)
        super().__init__(self._M, "orbx_frustum", int(device_id))

    def project(self, points, obs, items, idx, nmp, log_scale_factor: float, nlevels: int, cos_limit: float = 0.5, sum_order: int = SUM_LTR,
                log_kind: int = LOG_DOUBLE, want_depth: bool = True, stream=None, out: Optional[FrustumResult] = None,
                npoints: Optional[int] = None, nitems: Optional[int] = None, mcap: Optional[int] = None) -> FrustumResult:
        """orbx_frustum_project_device: `points` [M] records of TABLE_DTYPE (a [M, 48] uint8 or [M, 12] float32 tensor), `obs` [M] int32,
        `items` [B] records of ITEM_DTYPE (a [B, 112] uint8 or [B, 28] float32 tensor), `idx` [B, mcap] int32 and `nmp` [B] int32 on the
        device; asynchronous on `stream` (None or 0: the handle's own).  Without `out` the results are allocated on idx's device (torch):
        mp as [B, mcap, 32] uint8, what LocalMatchBatch.search_device takes."""
        M = int(points.shape[0]) if npoints is None else int(npoints)
        B = int(idx.shape[0]) if nitems is None else int(nitems)
        Q = int(idx.shape[1]) if mcap is None else int(mcap)
        if out is None:
            import torch
            dev = idx.device if hasattr(idx, "device") else torch.device("cuda", self.device_id)
            out = FrustumResult(torch.empty((B, Q, 32), dtype=torch.uint8, device=dev),
                                torch.empty((B, Q), dtype=torch.float32, device=dev) if want_depth else None,
                                torch.empty(B, dtype=torch.int32, device=dev))
        self._check(self._M.orbx_frustum_project_device(self._h, ptr(addr(points)), ptr(addr(obs)), M, ptr(addr(items)), B, ptr(addr(idx)),
                                                        ptr(addr(nmp)), Q, float(log_scale_factor), int(nlevels), float(cos_limit),
                                                        int(sum_order), int(log_kind), ptr(addr(out.mp)), ptr(addr(out.depth)),
                                                        ptr(addr(out.ntomatch)), ptr(int(stream or 0))))
        return out

    def project_host(self, points, obs, items, idx, nmp, log_scale_factor: float, nlevels: int, cos_limit: float = 0.5,
                     sum_order: int = SUM_LTR, log_kind: int = LOG_DOUBLE, want_depth: bool = True) -> FrustumResult:
        """orbx_frustum_project on numpy arrays of the same layout; returns when the results are on the host."""
        points, obs, items, idx, nmp, B, Q = _host_call(points, obs, items, idx, nmp)
        out = FrustumResult(np.zeros((B, Q), POINT_DTYPE), np.zeros((B, Q), np.float32) if want_depth else None, np.zeros(B, np.int32))
        self._check(self._M.orbx_frustum_project(self._h, ptr(points), ptr(obs), len(points), ptr(items), B, ptr(idx), ptr(nmp), Q,
                                                 float(log_scale_factor), int(nlevels), float(cos_limit), int(sum_order), int(log_kind),
                                                 ptr(out.mp), ptr(out.depth), ptr(out.ntomatch)))
        return out
