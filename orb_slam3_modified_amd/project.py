"""The Sophus Tcw * x projection fronts over liborbx_project.so (include/orbx_project.h): the projections of SearchByProjection(CurrentFrame,
LastFrame) (src/ORBmatcher.cc:1703-1721), of the relocalization SearchByProjection (:1913-1937) and of Fuse (:1198-1244) for B (pose, point
list) items at once over the table of map points FrustumBatch reads.  The rows they write are the records LastMatchBatch, ProjMatchBatch and
FuseBatch read, so `last(...).rows`, `reloc(...).rows` and `fuse(...).rows` go into `search_device` as they are.  All projection arithmetic
runs in the HIP kernels of the library (or, for the `reference_*` functions, in its plain C++ host twins); this file only marshals buffers."""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import _lib
from ._front import FrontHandle, ProjectResult, _fail, _host_call, _new, _sf, level_thresholds  # noqa: F401  (what sim3 shares)
from ._lib import addr, host_array as arr, ptr
from .frustum import LOG_DOUBLE, LOG_FLOAT, MAX_LEVELS, SUM_LTR, SUM_TREE, TABLE_DTYPE  # noqa: F401  (the table and the options of §24)
from .fuse import QUERY_DTYPE
from .lastmatch import POINT_DTYPE as LAST_POINT_DTYPE
from .projmatch import POINT_DTYPE as RELOC_POINT_DTYPE

ROT_MATRIX, ROT_QUAT = 0, 1
ITEM_DTYPE = np.dtype([("Rcw", "<f4", 9), ("tcw", "<f4", 3), ("Ow", "<f4", 3), ("q", "<f4", 4), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"),
                       ("cy", "<f4"), ("mbf", "<f4"), ("bounds", "<f4", 4), ("th", "<f4"), ("pad", "<f4", 3)])
SLOT_DTYPE = np.dtype([("point", "<i4"), ("octave", "<i4"), ("angle", "<f4"), ("pad", "<i4")])
assert ITEM_DTYPE.itemsize == 128 and SLOT_DTYPE.itemsize == 16


def reference_last(points, obs, items, slots, nslots, rot_kind: int = ROT_MATRIX, sum_order: int = SUM_LTR) -> ProjectResult:
    """orbx_project_last_reference: the host twin on numpy arrays (no device)."""
    M = _lib.project_lib()
    points, items, slots, nslots, B, Q = _host_call(points, items, slots, nslots, ITEM_DTYPE, SLOT_DTYPE)
    obs = arr(obs, np.int32, len(points))
    out = _new(B, Q, LAST_POINT_DTYPE)
    _fail(M.orbx_project_last_error, M.orbx_project_last_reference(ptr(points), ptr(obs), len(points), ptr(items), B, ptr(slots), ptr(nslots), Q,
                                                                   int(rot_kind), int(sum_order), ptr(out.rows), ptr(out.nvalid)))
    return out


def reference_reloc(points, items, slots, nslots, log_scale_factor: float, nlevels: int, log_kind: int = LOG_DOUBLE, rot_kind: int = ROT_MATRIX,
                    sum_order: int = SUM_LTR) -> ProjectResult:
    """orbx_project_reloc_reference: the host twin on numpy arrays (libm's log for every point, no thresholds, no device)."""
    M = _lib.project_lib()
    points, items, slots, nslots, B, Q = _host_call(points, items, slots, nslots, ITEM_DTYPE, SLOT_DTYPE)
    out = _new(B, Q, RELOC_POINT_DTYPE)
    _fail(M.orbx_project_last_error, M.orbx_project_reloc_reference(ptr(points), len(points), ptr(items), B, ptr(slots), ptr(nslots), Q,
                                                                    float(log_scale_factor), int(nlevels), int(log_kind), int(rot_kind),
                                                                    int(sum_order), ptr(out.rows), ptr(out.nvalid)))
    return out


def reference_fuse(points, items, idx, nslots, log_scale_factor: float, scale_factors, log_kind: int = LOG_DOUBLE, rot_kind: int = ROT_MATRIX,
                   sum_order: int = SUM_LTR) -> ProjectResult:
    """orbx_project_fuse_reference: the host twin on numpy arrays; nlevels is len(scale_factors)."""
    M = _lib.project_lib()
    points, items, idx, nslots, B, Q = _host_call(points, items, idx, nslots, ITEM_DTYPE)
    sf = _sf(scale_factors)
    out = _new(B, Q, QUERY_DTYPE)
    _fail(M.orbx_project_last_error, M.orbx_project_fuse_reference(ptr(points), len(points), ptr(items), B, ptr(idx), ptr(nslots), Q,
                                                                   float(log_scale_factor), ptr(sf), len(sf), int(log_kind), int(rot_kind),
                                                                   int(sum_order), ptr(out.rows), ptr(out.nvalid)))
    return out


class ProjectBatch(FrontHandle):
    """The projection fronts of TrackWithMotionModel, Relocalization and SearchInNeighbors for batches of (pose, point list) items; one
    handle holds one stream on one GPU."""

    def __init__(self, device_id: int = 0, library_path: Optional[str] = None):
        self._M = _lib.project_lib(library_path) if library_path else _lib.project_lib()
        self.device_id = int(device_id)
        super().__init__(self._M, "orbx_project", int(device_id))

    # ---- device forms: asynchronous on `stream` (None or 0: the handle's own); without `out` the results are allocated on the slots' device
    def last(self, points, obs, items, slots, nslots, rot_kind: int = ROT_MATRIX, sum_order: int = SUM_LTR, stream=None,
             out: Optional[ProjectResult] = None, npoints: Optional[int] = None, nitems: Optional[int] = None,
             mcap: Optional[int] = None) -> ProjectResult:
        """orbx_project_last_device: `points` [M] records of TABLE_DTYPE (a [M, 48] uint8 tensor), `obs` [M] int32, `items` [B] records of
        ITEM_DTYPE (a [B, 128] uint8 tensor), `slots` [B, mcap] records of SLOT_DTYPE (a [B, mcap, 16] uint8 tensor) and `nslots` [B] int32
        on the device.  rows: what LastMatchBatch.search_device takes as `points`."""
        M, B, Q = self._shape(points, slots, npoints, nitems, mcap)
        out = self._out(out, slots, B, Q, LAST_POINT_DTYPE)
        self._check(self._M.orbx_project_last_device(self._h, ptr(addr(points)), ptr(addr(obs)), M, ptr(addr(items)), B, ptr(addr(slots)),
                                                     ptr(addr(nslots)), Q, int(rot_kind), int(sum_order), ptr(addr(out.rows)),
                                                     ptr(addr(out.nvalid)), ptr(int(stream or 0))))
        return out

    def reloc(self, points, items, slots, nslots, log_scale_factor: float, nlevels: int, log_kind: int = LOG_DOUBLE, rot_kind: int = ROT_MATRIX,
              sum_order: int = SUM_LTR, stream=None, out: Optional[ProjectResult] = None, npoints: Optional[int] = None,
              nitems: Optional[int] = None, mcap: Optional[int] = None) -> ProjectResult:
        """orbx_project_reloc_device with the thresholds of (log_scale_factor, nlevels, log_kind).  rows: what ProjMatchBatch.search_device
        takes as `points` of items of kind 0."""
        M, B, Q = self._shape(points, slots, npoints, nitems, mcap)
        T = level_thresholds(log_scale_factor, nlevels, log_kind)
        out = self._out(out, slots, B, Q, RELOC_POINT_DTYPE)
        self._check(self._M.orbx_project_reloc_device(self._h, ptr(addr(points)), M, ptr(addr(items)), B, ptr(addr(slots)), ptr(addr(nslots)), Q,
                                                      ptr(T) if len(T) else None, int(nlevels), int(rot_kind), int(sum_order),
                                                      ptr(addr(out.rows)), ptr(addr(out.nvalid)), ptr(int(stream or 0))))
        return out

    def fuse(self, points, items, idx, nslots, log_scale_factor: float, scale_factors, log_kind: int = LOG_DOUBLE, rot_kind: int = ROT_MATRIX,
             sum_order: int = SUM_LTR, stream=None, out: Optional[ProjectResult] = None, npoints: Optional[int] = None,
             nitems: Optional[int] = None, mcap: Optional[int] = None) -> ProjectResult:
        """orbx_project_fuse_device: `idx` [B, mcap] int32 on the device, `scale_factors` a host array of nlevels floats.  rows: what
        FuseBatch.search_device takes as `query`."""
        M, B, Q = self._shape(points, idx, npoints, nitems, mcap)
        sf = _sf(scale_factors)
        T = level_thresholds(log_scale_factor, len(sf), log_kind)
        out = self._out(out, idx, B, Q, QUERY_DTYPE)
        self._check(self._M.orbx_project_fuse_device(self._h, ptr(addr(points)), M, ptr(addr(items)), B, ptr(addr(idx)), ptr(addr(nslots)), Q,
                                                     ptr(T) if len(T) else None, ptr(sf), len(sf), int(rot_kind), int(sum_order),
                                                     ptr(addr(out.rows)), ptr(addr(out.nvalid)), ptr(int(stream or 0))))
        return out

    # ---- host-array forms: numpy arrays of the same layout; they return when the results are on the host
    def last_host(self, points, obs, items, slots, nslots, rot_kind: int = ROT_MATRIX, sum_order: int = SUM_LTR) -> ProjectResult:
        """orbx_project_last."""
        points, items, slots, nslots, B, Q = _host_call(points, items, slots, nslots, ITEM_DTYPE, SLOT_DTYPE)
        obs = arr(obs, np.int32, len(points))
        out = _new(B, Q, LAST_POINT_DTYPE)
        self._check(self._M.orbx_project_last(self._h, ptr(points), ptr(obs), len(points), ptr(items), B, ptr(slots), ptr(nslots), Q, int(rot_kind),
                                              int(sum_order), ptr(out.rows), ptr(out.nvalid)))
        return out

    def reloc_host(self, points, items, slots, nslots, log_scale_factor: float, nlevels: int, log_kind: int = LOG_DOUBLE,
                   rot_kind: int = ROT_MATRIX, sum_order: int = SUM_LTR) -> ProjectResult:
        """orbx_project_reloc."""
        points, items, slots, nslots, B, Q = _host_call(points, items, slots, nslots, ITEM_DTYPE, SLOT_DTYPE)
        T = level_thresholds(log_scale_factor, nlevels, log_kind)
        out = _new(B, Q, RELOC_POINT_DTYPE)
        self._check(self._M.orbx_project_reloc(self._h, ptr(points), len(points), ptr(items), B, ptr(slots), ptr(nslots), Q,
                                               ptr(T) if len(T) else None, int(nlevels), int(rot_kind), int(sum_order), ptr(out.rows),
                                               ptr(out.nvalid)))
        return out

    def fuse_host(self, points, items, idx, nslots, log_scale_factor: float, scale_factors, log_kind: int = LOG_DOUBLE,
                  rot_kind: int = ROT_MATRIX, sum_order: int = SUM_LTR) -> ProjectResult:
        """orbx_project_fuse."""
        points, items, idx, nslots, B, Q = _host_call(points, items, idx, nslots, ITEM_DTYPE)
        sf = _sf(scale_factors)
        T = level_thresholds(log_scale_factor, len(sf), log_kind)
        out = _new(B, Q, QUERY_DTYPE)
        self._check(self._M.orbx_project_fuse(self._h, ptr(points), len(points), ptr(items), B, ptr(idx), ptr(nslots), Q,
                                              ptr(T) if len(T) else None, ptr(sf), len(sf), int(rot_kind), int(sum_order), ptr(out.rows),
                                              ptr(out.nvalid)))
        return out
