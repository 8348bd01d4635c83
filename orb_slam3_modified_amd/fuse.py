"""The batched Fuse search over liborbx_fuse.so (include/orbx_fuse.h): the window arg-min of ORBmatcher::Fuse (src/ORBmatcher.cc:1148), the
Sim3 Fuse (:1340) and SearchBySim3 (:1457) for P (query row, keyframe) pairs at once on the keypoints and descriptors a batch extraction
left in HBM.  All matching arithmetic runs in the HIP kernels of the library; this file only marshals buffers.  The caller projects its map
points (x, y, r, ur, the level range) and applies the side effects from best_idx / best_dist."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from ._lib import KP_DTYPE, OrbxFuseSide, addr, host_array as arr, host_view, ptr

LDS_MAX = 152 * 1024     # the largest LDS block of a workgroup (ORBX_FUSE_LDS lowers it)
MAX_CAPACITY = 32768
MAX_LEVELS = 16
QUERIES_PER_WORKGROUP = 512
QUERY_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("r", "<f4"), ("ur", "<f4"), ("min_level", "<i4"), ("max_level", "<i4"), ("point", "<i4"),
                        ("pad", "<i4")])
assert QUERY_DTYPE.itemsize == 32


def lds_bytes(capacity: int) -> int:
    """What the LDS path needs for a keyframe of this capacity: cell starts, records, indices, descriptors.  A search takes the LDS path
    when this is within the handle's limit, the global-memory path otherwise."""
    return 4 * (64 * 48 + 4) + 48 * capacity + 4 * ((capacity + 3) & ~3)


def grid_parameters(min_x, min_y, max_x, max_y) -> np.ndarray:
    """{min_x, min_y, inv_w, inv_h} of an image with these bounds, as Frame's constructor computes them (src/Frame.cc:153-160), float32."""
    f = np.float32
    return np.array([f(min_x), f(min_y), f(64) / (f(max_x) - f(min_x)), f(48) / (f(max_y) - f(min_y))], np.float32)


@dataclass
class FuseSide:
    """The keyframe side (orbx_fuse_side): kps [K, cap] keypoints (28 bytes each), desc [K, cap, 32], counts [K, 2], gridparm [K, 4]
    float32, uright [K, cap] float32 or None (monocular).  Torch tensors or raw HBM addresses for the device forms, numpy arrays for
    search."""
    kps: object
    desc: object
    counts: object
    gridparm: object
    nframes: int
    capacity: int
    uright: object = None

    def _struct(self) -> OrbxFuseSide:
        return OrbxFuseSide(*(addr(t) or None for t in (self.kps, self.desc, self.counts, self.uright, self.gridparm)), int(self.nframes),
                            int(self.capacity))

    def _host(self) -> "FuseSide":
        """Contiguous numpy arrays of the ABI's element types."""
        K, cap = int(self.nframes), int(self.capacity)
        kps = np.ascontiguousarray(self.kps)
        assert kps.nbytes == K * cap * KP_DTYPE.itemsize
        return FuseSide(kps, arr(self.desc, np.uint8, K, cap, 32), arr(self.counts, np.int32, K, 2), arr(self.gridparm, np.float32, K, 4), K, cap,
                        None if self.uright is None else arr(self.uright, np.float32, K, cap))


@dataclass
class FuseResult:
    """nfound [P] (queries with best_dist <= th_low; -1 for a malformed pair), best_idx / best_dist [P, qcap] (-1 / 256: no candidate); torch
    tensors from search_device, numpy arrays from search.  result[p] = (nfound, best_idx row, best_dist row) of pair p on the host."""
    nfound: object
    best_idx: object
    best_dist: object

    def __len__(self) -> int:
        return int(self.nfound.shape[0])

    def __getitem__(self, p: int):
        return int(host_view(self.nfound[p:p + 1])[0]), host_view(self.best_idx[p]), host_view(self.best_dist[p])


def _table(inv_level_sigma2):
    if inv_level_sigma2 is None:
        return None, None, 0
    s = np.ascontiguousarray(inv_level_sigma2, np.float32).ravel()
    return s, s.ctypes.data_as(C.POINTER(C.c_float)), len(s)


class FuseBatch(_lib.SideHandle):
    """Windowed nearest keypoints for batches of (query row, keyframe) pairs; one handle holds the grids of one side, one stream and its
    scratch on one GPU."""

    def __init__(self, device_id: int = 0):
        self._M = _lib.fuse_lib()
        self.device_id = int(device_id)
        super().__init__(self._M, "orbx_fuse", int(device_id))

    def grids_device(self, side: FuseSide, stream=None) -> None:
        """orbx_fuse_grids_device: the grids of the side's keyframes, kept in the handle until the next build; asynchronous on `stream`."""
        s = side._struct()
        self._check(self._M.orbx_fuse_grids_device(self._h, C.byref(s), ptr(int(stream or 0))))

    def search_device(self, side: FuseSide, query, nquery, pairs, pdesc, inv_level_sigma2=None, reprojection_gate: bool = False,
                      th_low: int = 50, stream=None, out: Optional[FuseResult] = None, npairs: Optional[int] = None,
                      qcap: Optional[int] = None, npoints: Optional[int] = None) -> FuseResult:
        """orbx_fuse_search_device after grids_device(side): `query` [P, qcap] records of QUERY_DTYPE (a [P, qcap, 32] uint8 tensor),
        `nquery` [P] int32, `pairs` [P] int32 and `pdesc` [M, 32] uint8 on the device, `inv_level_sigma2` a host array (needed with the gate);
        asynchronous on `stream` (None or 0: the handle's own).  Without `out` the result tensors are allocated on the pairs' device (torch)."""
        P = int(pairs.shape[0]) if npairs is None else int(npairs)
        Q = int(query.shape[1]) if qcap is None else int(qcap)
        M = int(pdesc.shape[0]) if npoints is None else int(npoints)
        if out is None:
            import torch
            dev = pairs.device if hasattr(pairs, "device") else torch.device("cuda", self.device_id)
            out = FuseResult(torch.empty(P, dtype=torch.int32, device=dev), torch.empty((P, Q), dtype=torch.int32, device=dev),
                             torch.empty((P, Q), dtype=torch.int32, device=dev))
        s = side._struct()
        _keep, pt, nl = _table(inv_level_sigma2)
        self._check(self._M.orbx_fuse_search_device(self._h, C.byref(s), ptr(addr(query)), ptr(addr(nquery)), Q, ptr(addr(pairs)), P,
                                                    ptr(addr(pdesc)), M, pt, nl, int(bool(reprojection_gate)), int(th_low), ptr(addr(out.best_idx)),
                                                    ptr(addr(out.best_dist)), ptr(addr(out.nfound)), ptr(int(stream or 0))))
        return out

    def search(self, side: FuseSide, query, nquery, pairs, pdesc, inv_level_sigma2=None, reprojection_gate: bool = False,
               th_low: int = 50) -> FuseResult:
        """orbx_fuse_search on numpy arrays of the same layout (`query` [P, qcap] of QUERY_DTYPE); builds the grids of the uploaded side and
        returns when the results are on the host."""
        hs = side._host()
        query = np.ascontiguousarray(query, QUERY_DTYPE)
        P, Q = query.shape
        nquery, pairs = arr(nquery, np.int32, P), arr(pairs, np.int32, P)
        pdesc = np.ascontiguousarray(pdesc, np.uint8).reshape(-1, 32)
        out = FuseResult(np.zeros(P, np.int32), np.zeros((P, Q), np.int32), np.zeros((P, Q), np.int32))
        s = hs._struct()
        _keep, pt, nl = _table(inv_level_sigma2)
        self._check(self._M.orbx_fuse_search(self._h, C.byref(s), ptr(query), ptr(nquery), Q, ptr(pairs), P, ptr(pdesc), len(pdesc), pt, nl,
                                             int(bool(reprojection_gate)), int(th_low), ptr(out.best_idx), ptr(out.best_dist), ptr(out.nfound)))
        return out
