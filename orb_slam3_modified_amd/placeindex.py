"""Place recognition through a device inverted file over liborbx_placeindex.so (include/orbx_placeindex.h): the candidates PlaceBatch
gives, bit for bit, with the membership step a walk over the lists of the query's words.  The database stays the caller's PlaceDb: append
rows and raise `count` (the rows after the synced count are visited pair by pair until the next sync), erase with n[d] = -1.  All
arithmetic runs in the library; this file only marshals buffers."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib
from ._lib import addr, ptr
from .place import NBEST, PlaceDb, PlaceQueries, PlaceResult

MAX_WORDS = 1 << 24          # ORBX_PLACEINDEX_MAX_WORDS
SCAN_TILE = 2048             # kScanTile: words of one scan workgroup (ORBX_PLACEINDEX_SCAN_TILE lowers it at create)
COUNT_GROUP = 16             # 1 << kGroupShift: lanes that share one query word's list (ORBX_PLACEINDEX_GROUP at create)


class PlaceIndex(_lib.SideHandle):
    """The inverted file of one database on one GPU, for a vocabulary of `n_words` words (ids [0, n_words)); one handle holds the file, one
    stream and its scratch."""

    def __init__(self, n_words: int, device: int = 0):
        self._P = _lib.placeindex_lib()
        self.device_id, self.n_words = int(device), int(n_words)
        super().__init__(self._P, "orbx_placeindex", int(device), int(n_words))

    def sync_device(self, db: PlaceDb, stream: int = 0) -> None:
        """orbx_placeindex_sync_device: rebuilds the file from db.ids / db.n / db.count; asynchronous on `stream` (0: the handle's own)."""
        ds = db.struct()
        self._check(self._P.orbx_placeindex_sync_device(self._h, C.byref(ds), ptr(int(stream))))

    def query_device(self, kind: int, db: PlaceDb, q: PlaceQueries, ccap: int, n_candidates: int = 0, out: Optional[PlaceResult] = None,
                     stream: int = 0) -> PlaceResult:
        """orbx_placeindex_query_device: PlaceBatch.query_device through the file.  db.kf_score is updated in place."""
        if out is None:
            import torch
            dev = q.ids.device if hasattr(q.ids, "device") else torch.device("cuda", self.device_id)
            z = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)   # noqa: E731
            two = kind == NBEST
            out = PlaceResult(z(q.count, ccap), z(q.count), z(q.count, ccap) if two else None, z(q.count) if two else None, z(q.count, 4))
        ds, qs = db.struct(), q.struct()
        self._check(self._P.orbx_placeindex_query_device(self._h, int(kind), int(n_candidates), C.byref(ds), C.byref(qs), int(ccap),
                                                         ptr(addr(out.cand)), ptr(addr(out.ncand)), ptr(addr(out.merge)), ptr(addr(out.nmerge)),
                                                         ptr(addr(out.stats)), ptr(int(stream))))
        return out

    def query(self, kind: int, db: PlaceDb, q: PlaceQueries, ccap: int, n_candidates: int = 0) -> PlaceResult:
        """orbx_placeindex_query: upload, sync, query and read back on numpy arrays.  db.kf_score (float32) is updated; the handle is left
        unsynced."""
        nq = int(q.count)
        two = kind == NBEST
        out = PlaceResult(np.full((nq, ccap), -1, np.int32), np.zeros(nq, np.int32), np.full((nq, ccap), -1, np.int32) if two else None,
                          np.zeros(nq, np.int32) if two else None, np.zeros((nq, 4), np.int32))
        ds, qs = db.struct(), q.struct()
        self._check(self._P.orbx_placeindex_query(self._h, int(kind), int(n_candidates), C.byref(ds), C.byref(qs), int(ccap), ptr(out.cand),
                                                  ptr(out.ncand), ptr(out.merge), ptr(out.nmerge), ptr(out.stats)))
        return out
