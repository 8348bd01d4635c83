"""The batched MapPoint::ComputeDistinctiveDescriptors over liborbx_mpdesc.so (include/orbx_mpdesc.h, src/MapPoint.cc:329-403): for M map
points at once, of a point's N observed descriptors the one whose median Hamming distance to the others is least, on the descriptors a
batch extraction left in HBM.  All arithmetic runs in the HIP kernels of the library; this file only marshals buffers.  The caller lists
each point's observations in the reference's push order; the winners land as rows of a descriptor table, which is what
FuseBatch.search_device reads as `pdesc`."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import NamedTuple, Optional

import numpy as np

from . import _lib
from ._lib import OrbxMpdescSide, addr, host_array as arr, ptr

MAX_OBS = 1024               # ORBX_MPDESC_MAX_OBS: a point with more observations is malformed
SMALL_CAP = 64               # the largest N the lane-per-observation form can take
MID_CAP = 256                # the largest N the form with the distances in LDS can take
SMALL_MAX = 64               # the routing boundaries of a handle (ORBX_MPDESC_SMALL_MAX / ORBX_MPDESC_MID_MAX change them at create):
MID_MAX = 256                # N <= SMALL_MAX: a lane per observation; N <= MID_MAX: the LDS matrix; above: the distances are recomputed
POINTS_PER_WORKGROUP = 128   # the lane-per-observation form: consecutive points of one workgroup,
LANES_PER_PASS = 256         # and the flat observation indices of one of its passes
BEST_EMPTY, BEST_MALFORMED = -1, -2
OBS_DTYPE = np.dtype([("frame", "<i4"), ("row", "<i4")])
assert OBS_DTYPE.itemsize == 8


@dataclass
class DistinctSide:
    """The descriptor side (orbx_mpdesc_side): desc [K, cap, 32] uint8, counts [K, 2] int32.  Torch tensors or raw HBM addresses for
    select_device, numpy arrays for select."""
    desc: object
    counts: object
    nframes: int
    capacity: int

    def _struct(self) -> OrbxMpdescSide:
        return OrbxMpdescSide(addr(self.desc) or None, addr(self.counts) or None, int(self.nframes), int(self.capacity))


class DistinctResult(NamedTuple):
    """best [M] (the winner's index in the point's list; -1: no observation, -2: malformed), median [M] (the winner's median; -1 for
    both), desc [R, 32] (the table with the winners' rows written); torch tensors from select_device, numpy arrays from select."""
    best: object
    median: object
    desc: object


class DistinctBatch(_lib.SideHandle):
    """Least-median descriptors for batches of map points; one handle holds one stream and its scratch on one GPU."""

    def __init__(self, device_id: int = 0):
        self._M = _lib.mpdesc_lib()
        self.device_id = int(device_id)
        super().__init__(self._M, "orbx_mpdesc", int(device_id))

    def select_device(self, side: DistinctSide, obs, obs_start, out_rows=None, out=None, stream=None, best=None, median=None,
                      nobs: Optional[int] = None, npoints: Optional[int] = None, table_rows: Optional[int] = None) -> DistinctResult:
        """orbx_mpdesc_select_device: `obs` [nobs] records of OBS_DTYPE (an [nobs, 2] int32 tensor), `obs_start` [M + 1] int32, `out_rows`
        [M] int32 or None (point m's row is m) and `out` [R, 32] uint8 (the table; None: a zeroed one of M rows) on the device;
        asynchronous on `stream` (None or 0: the handle's own).  Without `best` / `median` the result tensors are allocated on the
        observations' device (torch)."""
        M = int(obs_start.shape[0]) - 1 if npoints is None else int(npoints)
        n = int(obs.shape[0]) if nobs is None else int(nobs)
        if out is None or best is None or median is None:
            import torch
            dev = obs.device if hasattr(obs, "device") else torch.device("cuda", self.device_id)
            if out is None:
                if out_rows is not None:
                    raise ValueError("out_rows needs the table they index: pass out")
                out = torch.zeros((M, 32), dtype=torch.uint8, device=dev)
            best = torch.empty(M, dtype=torch.int32, device=dev) if best is None else best
            median = torch.empty(M, dtype=torch.int32, device=dev) if median is None else median
        R = int(out.shape[0]) if table_rows is None else int(table_rows)
        s = side._struct()
        self._check(self._M.orbx_mpdesc_select_device(self._h, C.byref(s), ptr(addr(obs)), n, ptr(addr(obs_start)), M, ptr(addr(out_rows)),
                                                      ptr(addr(out)), R, ptr(addr(best)), ptr(addr(median)), ptr(int(stream or 0))))
        return DistinctResult(best, median, out)

    def select(self, side: DistinctSide, obs, obs_start, out_rows=None, out=None) -> DistinctResult:
        """orbx_mpdesc_select on numpy arrays of the same layout; returns when the results are on the host.  `out`: the table the winners
        are written into, in place (None: a zeroed one of M rows); the rows no point writes keep what they held."""
        K, cap = int(side.nframes), int(side.capacity)
        hs = DistinctSide(arr(side.desc, np.uint8, K, cap, 32), arr(side.counts, np.int32, K, 2), K, cap)
        obs = np.ascontiguousarray(obs, OBS_DTYPE).reshape(-1)
        obs_start = np.ascontiguousarray(obs_start, np.int32).reshape(-1)
        M = len(obs_start) - 1
        if out is None:
            if out_rows is not None:
                raise ValueError("out_rows needs the table they index: pass out")
            out = np.zeros((M, 32), np.uint8)
        if not (isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags.c_contiguous and out.ndim == 2 and out.shape[1] == 32):
            raise ValueError("out must be a contiguous [R, 32] uint8 array")
        rows = None if out_rows is None else arr(out_rows, np.int32, M)
        best, median = np.zeros(M, np.int32), np.zeros(M, np.int32)
        s = hs._struct()
        self._check(self._M.orbx_mpdesc_select(self._h, C.byref(s), ptr(obs), len(obs), ptr(obs_start), M, ptr(rows), ptr(out), len(out),
                                               ptr(best), ptr(median)))
        return DistinctResult(best, median, out)
