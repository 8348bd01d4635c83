"""The batched MapPoint::UpdateNormalAndDepth over liborbx_mpgeom.so (include/orbx_mpgeom.h, src/MapPoint.cc:426-494): for M map points at
once, the view direction and the scale-invariance range, written in place into the table of map points FrustumBatch, ProjectBatch and
Sim3Batch read (frustum.TABLE_DTYPE).  All arithmetic runs in the HIP kernels of the library (or, for `reference`, in its plain C++ host
twin); this file only marshals buffers.  The caller lists each point's observations in the reference's loop order -- bad keyframes included,
unlike DistinctBatch's list -- and names the reference keyframe's row."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import NamedTuple, Optional

import numpy as np

from . import _lib
from ._lib import KP_DTYPE, OrbxError, OrbxMpgeomSide, addr, host_array as arr, ptr
from .frustum import SUM_LTR, SUM_TREE, TABLE_DTYPE  # noqa: F401
from .mpdesc import OBS_DTYPE

MAX_OBS = 1024               # ORBX_MPGEOM_MAX_OBS: a point with more observations is malformed
MAX_LEVELS = 16
DIV_QUOTIENT, DIV_RECIPROCAL = 0, 1
SMALL_CAP = 64               # kSmallCap: the largest N the lane-per-observation form can take
SMALL_MAX = 16               # kSmallDefault: a handle's routing boundary (ORBX_MPGEOM_SMALL_MAX changes it at create); above it: a wave per point
POINTS_PER_WAVE = 16         # the lane-per-observation form: consecutive points of one wave
N_MALFORMED = -2


@dataclass
class NormalDepthSide:
    """The side (orbx_mpgeom_side): kps [K, cap] records of KP_DTYPE, counts [K, 2] int32, nleft [K] int32 or None, centres [K, 8]
    float32.  Torch tensors or raw HBM addresses for update_device, numpy arrays for update and reference."""
    kps: object
    counts: object
    centres: object
    nframes: int
    capacity: int
    nleft: object = None

    def _struct(self) -> OrbxMpgeomSide:
        return OrbxMpgeomSide(addr(self.kps) or None, addr(self.counts) or None, addr(self.nleft) or None, addr(self.centres) or None,
                              int(self.nframes), int(self.capacity))

    def _host(self) -> "NormalDepthSide":
        K, cap = int(self.nframes), int(self.capacity)
        return NormalDepthSide(np.ascontiguousarray(self.kps, KP_DTYPE).reshape(K, cap), arr(self.counts, np.int32, K, 2),
                               arr(self.centres, np.float32, K, 8), K, cap, None if self.nleft is None else arr(self.nleft, np.int32, K))


class NormalDepthResult(NamedTuple):
    """n [M] (the observations counted; 0: none, -2: malformed), min_dist [M] (the raw mfMinDistance) or None, table (the table with the
    points' rows updated); torch tensors from update_device, numpy arrays from update and reference."""
    n: object
    min_dist: object
    table: object


def _sf(scale_factors) -> np.ndarray:
    return np.ascontiguousarray(scale_factors, np.float32).reshape(-1)


def _host_call(side, obs, obs_start, ref, rows, table, min_dist):
    hs = side._host()
    obs = np.ascontiguousarray(obs, OBS_DTYPE).reshape(-1)
    obs_start = np.ascontiguousarray(obs_start, np.int32).reshape(-1)
    M = len(obs_start) - 1
    ref = np.ascontiguousarray(ref, OBS_DTYPE).reshape(-1)
    if len(ref) != M:
        raise ValueError("ref must hold one record a point")
    if not (isinstance(table, np.ndarray) and table.dtype == TABLE_DTYPE and table.flags.c_contiguous and table.ndim == 1):
        raise ValueError("table must be a contiguous [R] array of TABLE_DTYPE")
    rows = None if rows is None else arr(rows, np.int32, M)
    if min_dist is None:
        min_dist = np.zeros(M, np.float32)
    elif not (isinstance(min_dist, np.ndarray) and min_dist.dtype == np.float32 and min_dist.flags.c_contiguous and min_dist.shape == (M,)):
        raise ValueError("min_dist must be a contiguous [M] float32 array")
    return hs, obs, obs_start, M, ref, rows, min_dist


def reference(side: NormalDepthSide, obs, obs_start, ref, table, scale_factors, rows=None, sum_order: int = SUM_LTR,
              div_kind: int = DIV_QUOTIENT, min_dist=None) -> NormalDepthResult:
    """orbx_mpgeom_update_reference: the host twin on numpy arrays, no device.  `table` is updated in place."""
    L = _lib.mpgeom_lib()
    hs, obs, obs_start, M, ref, rows, min_dist = _host_call(side, obs, obs_start, ref, rows, table, min_dist)
    sf, n = _sf(scale_factors), np.zeros(M, np.int32)
    s = hs._struct()
    rc = L.orbx_mpgeom_update_reference(C.byref(s), ptr(obs), len(obs), ptr(obs_start), M, ptr(ref), ptr(rows), ptr(table), len(table), ptr(sf),
                                        len(sf), int(sum_order), int(div_kind), ptr(n), ptr(min_dist))
    if rc < 0:
        raise OrbxError(rc, (L.orbx_mpgeom_last_error(None) or b"").decode())
    return NormalDepthResult(n, min_dist, table)


class NormalDepthBatch(_lib.SideHandle):
    """Normals and depth ranges for batches of map points; one handle holds one stream and its scratch on one GPU."""

    def __init__(self, device_id: int = 0, library_path: Optional[str] = None):
        self._M = _lib.mpgeom_lib(library_path) if library_path else _lib.mpgeom_lib()
        self.device_id = int(device_id)
        super().__init__(self._M, "orbx_mpgeom", int(device_id))

    def update_device(self, side: NormalDepthSide, obs, obs_start, ref, table, scale_factors, rows=None, sum_order: int = SUM_LTR,
                      div_kind: int = DIV_QUOTIENT, stream=None, n=None, min_dist=None, want_min_dist: bool = True, nobs: Optional[int] = None,
                      npoints: Optional[int] = None, table_rows: Optional[int] = None) -> NormalDepthResult:
        """orbx_mpgeom_update_device: `obs` [nobs] records of OBS_DTYPE (an [nobs, 2] int32 tensor), `obs_start` [M + 1] int32, `ref` [M]
        records of OBS_DTYPE, `rows` [M] int32 or None (point m's row is m) and `table` [R] records of TABLE_DTYPE (an [R, 48] uint8 or
        [R, 12] float32 tensor), updated in place, on the device; `scale_factors` host floats.  Asynchronous on `stream` (None or 0: the
        handle's own).  Without `n` / `min_dist` the result tensors are allocated on the observations' device (torch)."""
        M = int(obs_start.shape[0]) - 1 if npoints is None else int(npoints)
        k = int(obs.shape[0]) if nobs is None else int(nobs)
        R = int(table.shape[0]) if table_rows is None else int(table_rows)
        if n is None or (min_dist is None and want_min_dist):
            import torch
            dev = obs.device if hasattr(obs, "device") else torch.device("cuda", self.device_id)
            n = torch.empty(M, dtype=torch.int32, device=dev) if n is None else n
            if min_dist is None and want_min_dist:
                min_dist = torch.zeros(M, dtype=torch.float32, device=dev)
        sf = _sf(scale_factors)
        s = side._struct()
        self._check(self._M.orbx_mpgeom_update_device(self._h, C.byref(s), ptr(addr(obs)), k, ptr(addr(obs_start)), M, ptr(addr(ref)),
                                                      ptr(addr(rows)), ptr(addr(table)), R, ptr(sf), len(sf), int(sum_order), int(div_kind),
                                                      ptr(addr(n)), ptr(addr(min_dist)), ptr(int(stream or 0))))
        return NormalDepthResult(n, min_dist, table)

    def update(self, side: NormalDepthSide, obs, obs_start, ref, table, scale_factors, rows=None, sum_order: int = SUM_LTR,
               div_kind: int = DIV_QUOTIENT, min_dist=None) -> NormalDepthResult:
        """orbx_mpgeom_update on numpy arrays of the same layout; returns when the results are on the host.  `table` is updated in place;
        the rows no point writes, and every `pos` and `pad`, keep what they held.  `min_dist`: the array a malformed or empty point leaves
        as it was (None: zeros)."""
        hs, obs, obs_start, M, ref, rows, min_dist = _host_call(side, obs, obs_start, ref, rows, table, min_dist)
        sf, n = _sf(scale_factors), np.zeros(M, np.int32)
        s = hs._struct()
        self._check(self._M.orbx_mpgeom_update(self._h, C.byref(s), ptr(obs), len(obs), ptr(obs_start), M, ptr(ref), ptr(rows), ptr(table),
                                               len(table), ptr(sf), len(sf), int(sum_order), int(div_kind), ptr(n), ptr(min_dist)))
        return NormalDepthResult(n, min_dist, table)
