"""The projection fronts of LoopClosing's matcher callers over liborbx_sim3.so (include/orbx_sim3.h): the projections of the two Sim3
SearchByProjection overloads (src/ORBmatcher.cc:427, :534), of the Sim3 Fuse (:1340) and of both directions of SearchBySim3 (:1457), for B
items at once over the table of map points FrustumBatch and ProjectBatch read, and SearchBySim3's mutual-agreement pass (:1655-1671).  The
rows they write are the records ProjMatchBatch (items of KIND_SIM3) and FuseBatch (the reprojection gate off) read, so `proj(...).rows`,
`fuse(...).rows` and `search(...).rows` go into `search_device` as they are, and `search_by_sim3` chains a whole batch of SearchBySim3 calls
on the device.  All arithmetic runs in the HIP kernels of the library (or, for the `reference_*` functions, in its plain C++ host twins);
this file only marshals buffers."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from ._front import FrontHandle, ProjectResult, _fail, _host_call, _new, _sf, level_thresholds  # noqa: F401
from ._lib import addr, host_array as arr, host_view, ptr
from .frustum import LOG_DOUBLE, LOG_FLOAT, MAX_LEVELS, SUM_LTR, SUM_TREE, TABLE_DTYPE  # noqa: F401  (the table and the options of §24)
from .fuse import QUERY_DTYPE
from .project import ITEM_DTYPE as POSE_ITEM_DTYPE, ROT_MATRIX, ROT_QUAT  # noqa: F401  (§25's item and options)
from .projmatch import POINT_DTYPE

SIM3_MATRIX, SIM3_QUAT = 0, 1
PROJ_DIVIDE, PROJ_INVZ = 0, 1      # how proj projects: :427 (Pinhole::project) or :534 (invz, as SearchBySim3)
TH_HIGH = 100
ITEM_DTYPE = np.dtype([("Raw", "<f4", 9), ("taw", "<f4", 3), ("qa", "<f4", 4), ("s", "<f4"), ("Rba", "<f4", 9), ("tba", "<f4", 3), ("qba", "<f4", 4),
                       ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("bounds", "<f4", 4), ("th", "<f4"), ("pad", "<f4", 2)])
assert ITEM_DTYPE.itemsize == 176 and POSE_ITEM_DTYPE.itemsize == 128


@dataclass
class AgreeResult:
    """match12 [P, qcap] int32 (the keypoint of keyframe 2 agreed for keypoint i1 of keyframe 1, or -1) and nfound [P] int32 (what
    SearchBySim3 returns; -1 for a malformed pair); torch tensors from the device form, numpy arrays otherwise."""
    match12: object
    nfound: object

    def host(self) -> "AgreeResult":
        return AgreeResult(host_view(self.match12), host_view(self.nfound))


def _agree_call(best_idx12, best_dist12, nfound12, best_idx21, best_dist21, nfound21, n1, n2):
    i12 = np.ascontiguousarray(best_idx12, np.int32)
    P, Q = i12.shape
    blocks = (i12, arr(best_dist12, np.int32, P, Q), arr(nfound12, np.int32, P), arr(best_idx21, np.int32, P, Q), arr(best_dist21, np.int32, P, Q),
              arr(nfound21, np.int32, P), arr(n1, np.int32, P), arr(n2, np.int32, P))
    return blocks, P, Q


def reference_proj(points, items, idx, nslots, log_scale_factor: float, nlevels: int, log_kind: int = LOG_DOUBLE, rot_kind: int = ROT_MATRIX,
                   sum_order: int = SUM_LTR, proj_kind: int = PROJ_DIVIDE) -> ProjectResult:
    """orbx_sim3_proj_reference: the host twin on numpy arrays (libm's log for every point, no thresholds, no device)."""
    M = _lib.sim3_lib()
    points, items, idx, nslots, B, Q = _host_call(points, items, idx, nslots, POSE_ITEM_DTYPE)
    out = _new(B, Q, POINT_DTYPE)
    _fail(M.orbx_sim3_last_error, M.orbx_sim3_proj_reference(ptr(points), len(points), ptr(items), B, ptr(idx), ptr(nslots), Q, float(log_scale_factor),
                                                             int(nlevels), int(log_kind), int(proj_kind), int(rot_kind), int(sum_order), ptr(out.rows),
                                                             ptr(out.nvalid)))
    return out


def reference_fuse(points, items, idx, nslots, log_scale_factor: float, scale_factors, log_kind: int = LOG_DOUBLE, rot_kind: int = ROT_MATRIX,
                   sum_order: int = SUM_LTR) -> ProjectResult:
    """orbx_sim3_fuse_reference: the host twin on numpy arrays; nlevels is len(scale_factors)."""
    M = _lib.sim3_lib()
    points, items, idx, nslots, B, Q = _host_call(points, items, idx, nslots, POSE_ITEM_DTYPE)
    sf = _sf(scale_factors)
    out = _new(B, Q, QUERY_DTYPE)
    _fail(M.orbx_sim3_last_error, M.orbx_sim3_fuse_reference(ptr(points), len(points), ptr(items), B, ptr(idx), ptr(nslots), Q, float(log_scale_factor),
                                                             ptr(sf), len(sf), int(log_kind), int(rot_kind), int(sum_order), ptr(out.rows), ptr(out.nvalid)))
    return out


def reference_search(points, items, idx, nslots, log_scale_factor: float, scale_factors, log_kind: int = LOG_DOUBLE, rot_kind: int = ROT_MATRIX,
                     sum_order: int = SUM_LTR, sim_kind: int = SIM3_MATRIX) -> ProjectResult:
    """orbx_sim3_search_reference: the host twin on numpy arrays; `items` [B] records of ITEM_DTYPE, one per direction."""
    M = _lib.sim3_lib()
    points, items, idx, nslots, B, Q = _host_call(points, items, idx, nslots, ITEM_DTYPE)
    sf = _sf(scale_factors)
    out = _new(B, Q, QUERY_DTYPE)
    _fail(M.orbx_sim3_last_error, M.orbx_sim3_search_reference(ptr(points), len(points), ptr(items), B, ptr(idx), ptr(nslots), Q, float(log_scale_factor),
                                                               ptr(sf), len(sf), int(log_kind), int(rot_kind), int(sum_order), int(sim_kind), ptr(out.rows),
                                                               ptr(out.nvalid)))
    return out


def reference_agree(best_idx12, best_dist12, nfound12, best_idx21, best_dist21, nfound21, n1, n2, th_high: int = TH_HIGH) -> AgreeResult:
    """orbx_sim3_agree_reference: the agreement loop in plain C++ on numpy arrays (no device)."""
    M = _lib.sim3_lib()
    blocks, P, Q = _agree_call(best_idx12, best_dist12, nfound12, best_idx21, best_dist21, nfound21, n1, n2)
    out = AgreeResult(np.zeros((P, Q), np.int32), np.zeros(P, np.int32))
    _fail(M.orbx_sim3_last_error, M.orbx_sim3_agree_reference(*(ptr(b) for b in blocks), P, Q, int(th_high), ptr(out.match12), ptr(out.nfound)))
    return out


class Sim3Batch(FrontHandle):
    """The projection fronts of LoopClosing's matcher calls for batches of (pose or similarity, point list) items, and SearchBySim3's
    agreement pass; one handle holds one stream on one GPU."""

    def __init__(self, device_id: int = 0, library_path: Optional[str] = None):
        self._M = _lib.sim3_lib(library_path) if library_path else _lib.sim3_lib()
        self.device_id = int(device_id)
        super().__init__(self._M, "orbx_sim3", int(device_id))

    # ---- device forms: asynchronous on `stream` (None or 0: the handle's own); without `out` the results are allocated on the indices' device
    def proj(self, points, items, idx, nslots, log_scale_factor: float, nlevels: int, log_kind: int = LOG_DOUBLE, rot_kind: int = ROT_MATRIX,
             sum_order: int = SUM_LTR, proj_kind: int = PROJ_DIVIDE, stream=None, out: Optional[ProjectResult] = None, npoints: Optional[int] = None,
             nitems: Optional[int] = None, mcap: Optional[int] = None) -> ProjectResult:
        """orbx_sim3_proj_device with the thresholds of (log_scale_factor, nlevels, log_kind): `points` [M] records of TABLE_DTYPE (a [M, 48]
        uint8 tensor), `items` [B] records of POSE_ITEM_DTYPE (a [B, 128] uint8 tensor), `idx` [B, mcap] int32 and `nslots` [B] int32 on the
        device; `proj_kind` PROJ_DIVIDE for the overload of :427, PROJ_INVZ for the vpPointsKFs overload of :534.  rows: what
        ProjMatchBatch.search_device takes as `points` of items of KIND_SIM3."""
        M, B, Q = self._shape(points, idx, npoints, nitems, mcap)
        T = level_thresholds(log_scale_factor, nlevels, log_kind)
        out = self._out(out, idx, B, Q, POINT_DTYPE)
        self._check(self._M.orbx_sim3_proj_device(self._h, ptr(addr(points)), M, ptr(addr(items)), B, ptr(addr(idx)), ptr(addr(nslots)), Q,
                                                  ptr(T) if len(T) else None, int(nlevels), int(proj_kind), int(rot_kind), int(sum_order),
                                                  ptr(addr(out.rows)), ptr(addr(out.nvalid)), ptr(int(stream or 0))))
        return out

    def fuse(self, points, items, idx, nslots, log_scale_factor: float, scale_factors, log_kind: int = LOG_DOUBLE, rot_kind: int = ROT_MATRIX,
             sum_order: int = SUM_LTR, stream=None, out: Optional[ProjectResult] = None, npoints: Optional[int] = None,
             nitems: Optional[int] = None, mcap: Optional[int] = None) -> ProjectResult:
        """orbx_sim3_fuse_device: `scale_factors` a host array of nlevels floats.  rows: what FuseBatch.search_device takes as `query`, with
        reprojection_gate=False."""
        M, B, Q = self._shape(points, idx, npoints, nitems, mcap)
        sf = _sf(scale_factors)
        T = level_thresholds(log_scale_factor, len(sf), log_kind)
        out = self._out(out, idx, B, Q, QUERY_DTYPE)
        self._check(self._M.orbx_sim3_fuse_device(self._h, ptr(addr(points)), M, ptr(addr(items)), B, ptr(addr(idx)), ptr(addr(nslots)), Q,
                                                  ptr(T) if len(T) else None, ptr(sf), len(sf), int(rot_kind), int(sum_order), ptr(addr(out.rows)),
                                                  ptr(addr(out.nvalid)), ptr(int(stream or 0))))
        return out

    def search(self, points, items, idx, nslots, log_scale_factor: float, scale_factors, log_kind: int = LOG_DOUBLE, rot_kind: int = ROT_MATRIX,
               sum_order: int = SUM_LTR, sim_kind: int = SIM3_MATRIX, stream=None, out: Optional[ProjectResult] = None,
               npoints: Optional[int] = None, nitems: Optional[int] = None, mcap: Optional[int] = None) -> ProjectResult:
        """orbx_sim3_search_device: `items` [B] records of ITEM_DTYPE (a [B, 176] uint8 tensor), one per direction; slot j of `idx` is the map
        point of keypoint j of the source keyframe.  rows: what FuseBatch.search_device takes as `query`, with reprojection_gate=False."""
        M, B, Q = self._shape(points, idx, npoints, nitems, mcap)
        sf = _sf(scale_factors)
        T = level_thresholds(log_scale_factor, len(sf), log_kind)
        out = self._out(out, idx, B, Q, QUERY_DTYPE)
        self._check(self._M.orbx_sim3_search_device(self._h, ptr(addr(points)), M, ptr(addr(items)), B, ptr(addr(idx)), ptr(addr(nslots)), Q,
                                                    ptr(T) if len(T) else None, ptr(sf), len(sf), int(rot_kind), int(sum_order), int(sim_kind),
                                                    ptr(addr(out.rows)), ptr(addr(out.nvalid)), ptr(int(stream or 0))))
        return out

    def agree(self, best_idx12, best_dist12, nfound12, best_idx21, best_dist21, nfound21, n1, n2, th_high: int = TH_HIGH, stream=None,
              out: Optional[AgreeResult] = None, npairs: Optional[int] = None, qcap: Optional[int] = None) -> AgreeResult:
        """orbx_sim3_agree_device on the blocks two FuseBatch.search_device calls wrote ([P, qcap] int32 and [P] int32 on the device) and the
        keyframes' keypoint counts `n1`, `n2` [P] int32."""
        P = int(best_idx12.shape[0]) if npairs is None else int(npairs)
        Q = int(best_idx12.shape[1]) if qcap is None else int(qcap)
        if out is None:
            import torch
            dev = self._dev(best_idx12)
            out = AgreeResult(torch.empty((P, Q), dtype=torch.int32, device=dev), torch.empty(P, dtype=torch.int32, device=dev))
        self._check(self._M.orbx_sim3_agree_device(self._h, *(ptr(addr(b)) for b in (best_idx12, best_dist12, nfound12, best_idx21, best_dist21,
                                                                                      nfound21, n1, n2)), P, Q, int(th_high),
                                                   ptr(addr(out.match12)), ptr(addr(out.nfound)), ptr(int(stream or 0))))
        return out

    def search_by_sim3(self, fuse_batch, side, points, items12, items21, idx1, n1, idx2, n2, kf1, kf2, pdesc, log_scale_factor: float,
                       scale_factors, log_kind: int = LOG_DOUBLE, rot_kind: int = ROT_MATRIX, sum_order: int = SUM_LTR,
                       sim_kind: int = SIM3_MATRIX, th_high: int = TH_HIGH, stream=None) -> AgreeResult:
        """A batch of P SearchBySim3 calls on the device, after fuse_batch.grids_device(side): the two directions' projections, two
        FuseBatch searches with the reprojection gate off, and the agreement pass; nothing leaves the device.  The chain spans two
        handles, whose own streams do not wait for each other, so all five calls go to ONE stream: `stream` when given (asynchronous on
        it; the grids must have been built on it or be complete), else a stream this batch keeps for its chains, which first waits for
        the device's pending work (the grids, the caller's uploads) and is synchronized before the call returns.
        `items12` [P] (T_1w, S21, the bounds of keyframe 2) and `items21` [P] (T_2w, S12, the bounds of keyframe 1) records of ITEM_DTYPE;
        `idx1`, `idx2` [P, qcap] int32: the map point of each keypoint of keyframe 1 / 2 (negative: none, bad or already matched) with
        `n1`, `n2` [P] their keypoint counts; `kf1`, `kf2` [P] int32 the keyframes' rows in `side`; `pdesc` [M, 32] the points'
        descriptors, row for row with `points`."""
        own = None
        if not stream:
            import torch
            if getattr(self, "_chain_stream", None) is None:
                self._chain_stream = torch.cuda.Stream(device=self._dev(idx1))
            own = self._chain_stream
            torch.cuda.synchronize(own.device)      # what the caller queued on any stream, the handles' own included, is done
            stream = own.cuda_stream
        q12 = self.search(points, items12, idx1, n1, log_scale_factor, scale_factors, log_kind, rot_kind, sum_order, sim_kind, stream=stream)
        q21 = self.search(points, items21, idx2, n2, log_scale_factor, scale_factors, log_kind, rot_kind, sum_order, sim_kind, stream=stream)
        r12 = fuse_batch.search_device(side, q12.rows, n1, kf2, pdesc, None, False, th_high, stream=stream)
        r21 = fuse_batch.search_device(side, q21.rows, n2, kf1, pdesc, None, False, th_high, stream=stream)
        out = self.agree(r12.best_idx, r12.best_dist, r12.nfound, r21.best_idx, r21.best_dist, r21.nfound, n1, n2, th_high, stream=stream)
        if own is not None:
            own.synchronize()
        return out

    # ---- host-array forms: numpy arrays of the same layout; they return when the results are on the host
    def proj_host(self, points, items, idx, nslots, log_scale_factor: float, nlevels: int, log_kind: int = LOG_DOUBLE, rot_kind: int = ROT_MATRIX,
                  sum_order: int = SUM_LTR, proj_kind: int = PROJ_DIVIDE) -> ProjectResult:
        """orbx_sim3_proj."""
        points, items, idx, nslots, B, Q = _host_call(points, items, idx, nslots, POSE_ITEM_DTYPE)
        T = level_thresholds(log_scale_factor, nlevels, log_kind)
        out = _new(B, Q, POINT_DTYPE)
        self._check(self._M.orbx_sim3_proj(self._h, ptr(points), len(points), ptr(items), B, ptr(idx), ptr(nslots), Q, ptr(T) if len(T) else None,
                                           int(nlevels), int(proj_kind), int(rot_kind), int(sum_order), ptr(out.rows), ptr(out.nvalid)))
        return out

    def fuse_host(self, points, items, idx, nslots, log_scale_factor: float, scale_factors, log_kind: int = LOG_DOUBLE, rot_kind: int = ROT_MATRIX,
                  sum_order: int = SUM_LTR) -> ProjectResult:
        """orbx_sim3_fuse."""
        points, items, idx, nslots, B, Q = _host_call(points, items, idx, nslots, POSE_ITEM_DTYPE)
        sf = _sf(scale_factors)
        T = level_thresholds(log_scale_factor, len(sf), log_kind)
        out = _new(B, Q, QUERY_DTYPE)
        self._check(self._M.orbx_sim3_fuse(self._h, ptr(points), len(points), ptr(items), B, ptr(idx), ptr(nslots), Q, ptr(T) if len(T) else None,
                                           ptr(sf), len(sf), int(rot_kind), int(sum_order), ptr(out.rows), ptr(out.nvalid)))
        return out

    def search_host(self, points, items, idx, nslots, log_scale_factor: float, scale_factors, log_kind: int = LOG_DOUBLE,
                    rot_kind: int = ROT_MATRIX, sum_order: int = SUM_LTR, sim_kind: int = SIM3_MATRIX) -> ProjectResult:
        """orbx_sim3_search."""
        points, items, idx, nslots, B, Q = _host_call(points, items, idx, nslots, ITEM_DTYPE)
        sf = _sf(scale_factors)
        T = level_thresholds(log_scale_factor, len(sf), log_kind)
        out = _new(B, Q, QUERY_DTYPE)
        self._check(self._M.orbx_sim3_search(self._h, ptr(points), len(points), ptr(items), B, ptr(idx), ptr(nslots), Q, ptr(T) if len(T) else None,
                                             ptr(sf), len(sf), int(rot_kind), int(sum_order), int(sim_kind), ptr(out.rows), ptr(out.nvalid)))
        return out

    def agree_host(self, best_idx12, best_dist12, nfound12, best_idx21, best_dist21, nfound21, n1, n2, th_high: int = TH_HIGH) -> AgreeResult:
        """orbx_sim3_agree."""
        blocks, P, Q = _agree_call(best_idx12, best_dist12, nfound12, best_idx21, best_dist21, nfound21, n1, n2)
        out = AgreeResult(np.zeros((P, Q), np.int32), np.zeros(P, np.int32))
        self._check(self._M.orbx_sim3_agree(self._h, *(ptr(b) for b in blocks), P, Q, int(th_high), ptr(out.match12), ptr(out.nfound)))
        return out
