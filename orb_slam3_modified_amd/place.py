"""Batched place recognition over liborbx_place.so (include/orbx_place.h): KeyFrameDatabase::DetectRelocalizationCandidates and
DetectNBestCandidates (src/KeyFrameDatabase.cc:733-845, :604-730) for Q query BowVectors against D keyframe BowVectors, both in the
fixed-stride device layout BowBatch.transform_device writes.  All arithmetic runs in the library; this file only marshals buffers."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import OrbxPlaceDb, OrbxPlaceQueries, addr, ptr

RELOC, NBEST = 0, 1          # ORBX_PLACE_RELOC, ORBX_PLACE_NBEST
COV = 10                     # ORBX_PLACE_COV: GetBestCovisibilityKeyFrames(10)
QUERY_LDS = 4096             # kPlaceLds: a query of at most this many entries is staged in LDS (ORBX_PLACE_LDS lowers it at create)
DB_PER_WORKGROUP = 32        # kTile: database vectors of one k_place_pairs workgroup, a wave per pair

BowVector = Tuple[np.ndarray, np.ndarray]


@dataclass
class PlaceDb:
    """orbx_place_db: torch tensors, numpy arrays (the host form) or raw addresses.  ids / vals [D, stride], n [D] (< 0: erased), kf_map [D],
    kf_cov [D, 10] rows padded with -1, kf_score [D] float32 (read and updated)."""
    ids: object
    vals: object
    n: object
    kf_map: object
    kf_cov: object
    kf_score: object
    count: int
    stride: int

    def struct(self) -> OrbxPlaceDb:
        return OrbxPlaceDb(addr(self.ids), addr(self.vals), addr(self.n), addr(self.kf_map), addr(self.kf_cov), addr(self.kf_score),
                           int(self.count), int(self.stride))


@dataclass
class PlaceQueries:
    """orbx_place_queries: ids / vals [Q, stride], n [Q], q_map [Q]; excl_ptr [Q + 1] and excl_idx [n_excl] (N-best: each query's excluded
    rows, strictly ascending) or None."""
    ids: object
    vals: object
    n: object
    q_map: object
    count: int
    stride: int
    excl_ptr: object = None
    excl_idx: object = None
    n_excl: int = 0

    def struct(self) -> OrbxPlaceQueries:
        return OrbxPlaceQueries(addr(self.ids), addr(self.vals), addr(self.n), addr(self.q_map), addr(self.excl_ptr), addr(self.excl_idx),
                                int(self.count), int(self.stride), int(self.n_excl))


@dataclass
class PlaceResult:
    """cand [Q, ccap] rows (-1 beyond the count), ncand [Q] (the full count; -1: a malformed query), merge / nmerge the same for
    vpMergeCand (N-best, else None), stats [Q, 4] = {rows in the query, scored rows, maxCommonWords, minCommonWords}."""
    cand: object
    ncand: object
    merge: object
    nmerge: object
    stats: object


def fixed_stride(vectors: Sequence[Optional[BowVector]], stride: int):
    """Host arrays of the device layout from a list of (ids, values); None: an erased row (count -1)."""
    n = len(vectors)
    ids, vals, counts = np.zeros((n, stride), np.uint32), np.zeros((n, stride), np.float64), np.zeros(n, np.int32)
    for i, v in enumerate(vectors):
        if v is None:
            counts[i] = -1
            continue
        k = len(v[0])
        ids[i, :k], vals[i, :k], counts[i] = v[0], v[1], k
    return ids, vals, counts


def exclusions(rows: Sequence[Sequence[int]]):
    """(excl_ptr, excl_idx, n_excl) from each query's excluded rows (any order; sorted here)."""
    p = np.zeros(len(rows) + 1, np.int32)
    for i, r in enumerate(rows):
        p[i + 1] = p[i] + len(set(r))
    idx = np.array([d for r in rows for d in sorted(set(r))], np.int32)
    return p, idx, len(idx)


class PlaceBatch(_lib.SideHandle):
    """Relocalization and N-best candidates of Q queries against one database; one handle holds one stream and its scratch on one GPU."""

    def __init__(self, device: int = 0):
        self._P = _lib.place_lib()
        self.device_id = int(device)
        super().__init__(self._P, "orbx_place", int(device))

    def query_device(self, kind: int, db: PlaceDb, q: PlaceQueries, ccap: int, n_candidates: int = 0, out: Optional[PlaceResult] = None,
                     stream: int = 0) -> PlaceResult:
        """orbx_place_query_device; asynchronous on `stream` (0: the handle's own).  Without `out` the result tensors are allocated with
        torch on the queries' device.  db.kf_score is updated in place."""
        if out is None:
            import torch
            dev = q.ids.device if hasattr(q.ids, "device") else torch.device("cuda", self.device_id)
            z = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)   # noqa: E731
            two = kind == NBEST
            out = PlaceResult(z(q.count, ccap), z(q.count), z(q.count, ccap) if two else None, z(q.count) if two else None, z(q.count, 4))
        ds, qs = db.struct(), q.struct()
        self._check(self._P.orbx_place_query_device(self._h, int(kind), int(n_candidates), C.byref(ds), C.byref(qs), int(ccap), ptr(addr(out.cand)),
                                                    ptr(addr(out.ncand)), ptr(addr(out.merge)), ptr(addr(out.nmerge)), ptr(addr(out.stats)),
                                                    ptr(int(stream))))
        return out

    def query(self, kind: int, db: PlaceDb, q: PlaceQueries, ccap: int, n_candidates: int = 0) -> PlaceResult:
        """orbx_place_query: the same on numpy arrays; returns when the results are in host memory.  db.kf_score (float32) is updated."""
        nq = int(q.count)
        two = kind == NBEST
        out = PlaceResult(np.full((nq, ccap), -1, np.int32), np.zeros(nq, np.int32), np.full((nq, ccap), -1, np.int32) if two else None,
                          np.zeros(nq, np.int32) if two else None, np.zeros((nq, 4), np.int32))
        ds, qs = db.struct(), q.struct()
        self._check(self._P.orbx_place_query(self._h, int(kind), int(n_candidates), C.byref(ds), C.byref(qs), int(ccap), ptr(out.cand),
                                             ptr(out.ncand), ptr(out.merge), ptr(out.nmerge), ptr(out.stats)))
        return out
