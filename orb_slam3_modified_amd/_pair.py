"""What the bindings of the four pair matchers share (match, rigbow, trimatch, initmatch): a side's struct and its host conversion, a
result's rows, the results' allocation and the marshalling of a host call, beside csrc/side/orbx_pair_host.h."""
from __future__ import annotations

import dataclasses

import numpy as np

from ._lib import KP_DTYPE, addr, host_array as arr, host_view

# a side's arrays after kps: element type, shape for F frames of capacity cap, whether the array may be None
_ARRAYS = {"desc": (np.uint8, lambda F, cap: (F, cap, 32), False), "counts": (np.int32, lambda F, cap: (F, 2), False),
           "fv_node": (np.uint32, lambda F, cap: (F, cap), False), "fv_ptr": (np.int32, lambda F, cap: (F, cap + 1), False),
           "fv_feat": (np.uint32, lambda F, cap: (F, cap), False), "fv_n": (np.int32, lambda F, cap: (F,), False),
           "valid": (np.uint8, lambda F, cap: (F, cap), True), "nleft": (np.int32, lambda F, cap: (F,), True),
           "has_point": (np.uint8, lambda F, cap: (F, cap), True), "uright": (np.float32, lambda F, cap: (F, cap), True)}
FV = ("fv_node", "fv_ptr", "fv_feat", "fv_n")


class PairSide:
    """One side of the pairs.  A subclass is a dataclass with nframes, capacity and the arrays that `_FIELDS` names in the order of its
    structure `_STRUCT` (kps first)."""
    _STRUCT = None
    _FIELDS = ()

    def _struct(self):
        return self._STRUCT(*(addr(getattr(self, n)) or None for n in self._FIELDS), int(self.nframes), int(self.capacity))

    def _host(self):
        """Contiguous numpy arrays of the ABI's element types."""
        F, cap = int(self.nframes), int(self.capacity)
        kps = np.ascontiguousarray(self.kps)
        assert kps.nbytes == F * cap * KP_DTYPE.itemsize
        new = {"kps": kps}
        for n in self._FIELDS[1:]:
            dtype, shape, optional = _ARRAYS[n]
            new[n] = None if optional and getattr(self, n) is None else arr(getattr(self, n), dtype, *shape(F, cap))
        return dataclasses.replace(self, nframes=F, capacity=cap, **new)


class PairResult:
    """nmatches [P] and the rows that `_ROWS` names; result[p] = (nmatches, a row of each) of pair p on the host."""
    _ROWS = ()

    def __len__(self) -> int:
        return int(self.nmatches.shape[0])

    def __getitem__(self, p: int):
        return int(host_view(self.nmatches[p:p + 1])[0]), *(host_view(getattr(self, n)[p]) if getattr(self, n) is not None else None for n in self._ROWS)


def count(pairs, npairs) -> int:
    return int(pairs.shape[0]) if npairs is None else int(npairs)


def new_results(P: int, tails, handle=None, pairs=None) -> list:
    """One int32 array [P, *tail] per tail: numpy zeros for a host form; for the device form of `handle`, torch tensors on the pairs' device
    (the handle's when `pairs` is a raw address)."""
    if handle is None:
        return [np.zeros((P,) + tuple(t), np.int32) for t in tails]
    import torch
    dev = pairs.device if hasattr(pairs, "device") else torch.device("cuda", handle.device_id)
    return [torch.empty((P,) + tuple(t), dtype=torch.int32, device=dev) for t in tails]


def host_call(a: PairSide, b: PairSide, pairs):
    """A host form's arguments: both sides on the host (converted once when they are one object), pairs [P, 2] int32 and P."""
    ha = a._host()
    hb = ha if b is a else b._host()
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    return ha, hb, pairs, len(pairs)
