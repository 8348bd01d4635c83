"""What the bindings of the projection fronts share (project, sim3): the result record, the cached thresholds, the marshalling of a host
call and the device forms' allocation, beside csrc/side/orbx_front_host.h."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _lib, frustum
from ._lib import OrbxError, host_array as arr, host_view
from .frustum import LOG_DOUBLE, TABLE_DTYPE


@dataclass
class ProjectResult:
    """rows [B, mcap] records of the consumer's dtype (from the device forms: a [B, mcap, 32] uint8 torch tensor on the device) and nvalid [B]
    int32 (-1 for a malformed item)."""
    rows: object
    nvalid: object
    dtype: np.dtype

    def host(self) -> "ProjectResult":
        """The same on the host: rows as a [B, mcap] array of the consumer's dtype."""
        rows = host_view(self.rows)
        if rows.dtype != self.dtype:
            rows = np.ascontiguousarray(rows).view(self.dtype).reshape(rows.shape[0], rows.shape[1])
        return ProjectResult(rows, host_view(self.nvalid), self.dtype)


_thresholds = {}


def level_thresholds(log_scale_factor: float, nlevels: int, log_kind: int = LOG_DOUBLE) -> np.ndarray:
    """frustum.level_thresholds, computed once per (log_scale_factor, nlevels, log_kind): these libraries never bisect."""
    key = (np.float32(log_scale_factor).tobytes(), int(nlevels), int(log_kind))
    if key not in _thresholds:
        T = frustum.level_thresholds(log_scale_factor, nlevels, log_kind)
        T.setflags(write=False)
        _thresholds[key] = T
    return _thresholds[key]


def _host_call(points, items, slots, nslots, item_dtype, slot_dtype=np.int32):
    points = np.ascontiguousarray(points, TABLE_DTYPE).ravel()
    items = np.ascontiguousarray(items, item_dtype).ravel()
    slots = np.ascontiguousarray(slots, slot_dtype)
    B, Q = slots.shape
    assert len(items) == B
    return points, items, slots, arr(nslots, np.int32, B), B, Q


def _fail(last_error, rc):
    """Raise for a host twin's negative return; `last_error` is its library's orbx_*_last_error."""
    if rc < 0:
        raise OrbxError(rc, (last_error(None) or b"").decode())


def _sf(scale_factors) -> np.ndarray:
    return arr(scale_factors, np.float32, len(scale_factors))


def _new(B, Q, dtype) -> ProjectResult:
    return ProjectResult(np.zeros((B, Q), dtype), np.zeros(B, np.int32), dtype)


class FrontHandle(_lib.SideHandle):
    """A side handle whose device forms take [B, mcap] slots and write [B, mcap, 32] rows."""

    def _dev(self, like):
        import torch
        return like.device if hasattr(like, "device") else torch.device("cuda", self.device_id)

    def _out(self, out, like, B, Q, dtype):
        if out is not None:
            return out
        import torch
        dev = self._dev(like)
        return ProjectResult(torch.empty((B, Q, 32), dtype=torch.uint8, device=dev), torch.empty(B, dtype=torch.int32, device=dev), dtype)

    @staticmethod
    def _shape(points, slots, npoints, nitems, mcap):
        return (int(points.shape[0]) if npoints is None else int(npoints), int(slots.shape[0]) if nitems is None else int(nitems),
                int(slots.shape[1]) if mcap is None else int(mcap))
