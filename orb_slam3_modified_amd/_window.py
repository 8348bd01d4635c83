"""What the bindings of the four chained projection matchers share (localmatch, lastmatch, projmatch, rigmatch): the limits and the LDS
sizing of csrc/side/orbx_window_device.h (one grid: lds_bytes; the rig's two: rig_lds_bytes) and the level table's marshalling."""
from __future__ import annotations

import ctypes as C

import numpy as np

LDS_MAX = 148 * 1024     # the largest dynamic LDS block of a workgroup, kLdsMax (a library's ORBX_*_LDS lowers it)
MAX_CAPACITY = 32768
MAX_LEVELS = 16


def _up16(n: int) -> int:
    return (n + 15) & ~15


def _grid_bytes(capacity: int) -> int:
    """One camera's descriptors and grid_layout's block: sorted keys (a power of two of them), records, cell starts."""
    p2 = 2
    while p2 < capacity:
        p2 <<= 1
    return sum(_up16(b) for b in (32 * capacity, 4 * p2, 16 * capacity, 2 * (64 * 48 + 1)))


def lds_bytes(capacity: int, mcap: int) -> int:
    """layout(capacity, mcap, p2, true).fixed: what the LDS path needs beside the candidate room for frames of this capacity and rows of up
    to `mcap` points: descriptors, sorted keys, records, cell starts, offsets, the points' results.  A search takes the LDS path when this
    plus one list of `capacity` candidates is within the handle's limit; the rest of the limit is candidate room (4 bytes a candidate)."""
    return _grid_bytes(capacity) + _up16(4 * (mcap + 1)) + _up16(4 * mcap)


def rig_lds_bytes(cap_l: int, cap_r: int, mcap: int) -> int:
    """rig_layout(cap_l, cap_r, mcap, ..., true).fixed: both descriptor sets, both grids, the offsets of 2 mcap lists and four results a
    point.  A call takes the LDS path when this plus cap_l + cap_r candidates (one point's longest pair of lists) is within the handle's
    limit; the rest of the limit is candidate room (4 bytes a candidate)."""
    return _grid_bytes(cap_l) + _grid_bytes(cap_r) + _up16(4 * (2 * mcap + 1)) + _up16(16 * mcap)


def _table(scale_factors):
    s = np.ascontiguousarray(scale_factors, np.float32).ravel()
    return s, s.ctypes.data_as(C.POINTER(C.c_float)), len(s)
