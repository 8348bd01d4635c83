"""What the bindings of the three chained projection matchers share (localmatch, lastmatch, projmatch): the limits and the LDS sizing of
csrc/side/orbx_window_device.h and the level table's marshalling."""
from __future__ import annotations

import ctypes as C

import numpy as np

LDS_MAX = 148 * 1024     # the largest dynamic LDS block of a workgroup, kLdsMax (a library's ORBX_*_LDS lowers it)
MAX_CAPACITY = 32768
MAX_LEVELS = 16


def _up16(n: int) -> int:
    return (n + 15) & ~15


def lds_bytes(capacity: int, mcap: int) -> int:
    """layout(capacity, mcap, p2, true).fixed: what the LDS path needs beside the candidate room for frames of this capacity and rows of up
    to `mcap` points: descriptors, sorted keys, records, cell starts, offsets, the points' results.  A search takes the LDS path when this
    plus one list of `capacity` candidates is within the handle's limit; the rest of the limit is candidate room (4 bytes a candidate)."""
    p2 = 2
    while p2 < capacity:
        p2 <<= 1
    return sum(_up16(b) for b in (32 * capacity, 4 * p2, 16 * capacity, 2 * (64 * 48 + 1), 4 * (mcap + 1), 4 * mcap))


def _table(scale_factors):
    s = np.ascontiguousarray(scale_factors, np.float32).ravel()
    return s, s.ctypes.data_as(C.POINTER(C.c_float)), len(s)
