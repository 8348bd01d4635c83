"""All six DBoW2 scorings over liborbx_score.so (include/orbx_score.h, Thirdparty/DBoW2/DBoW2/ScoringObject.cpp): the score of one pair on
the host, and of every (query, database) pair of two batches of BowVectors on the GPU.  The scoring is an argument of every call (DBoW2's
ScoringType values); KL exists as a host pair only.  All arithmetic runs in the library; this file only marshals buffers."""
from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import addr, ptr

L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT = range(6)   # DBoW2::ScoringType
SCORINGS = (L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT)
DEVICE_SCORINGS = (L1_NORM, L2_NORM, CHI_SQUARE, BHATTACHARYYA, DOT_PRODUCT)   # KL needs glibc's log bit for bit: orbx_score_pair only
QUERY_LDS = 4096             # kScoreLds: a query of at most this many entries is staged in LDS (ORBX_SCORE_LDS lowers it at create)
DB_PER_WORKGROUP = 32        # kTile: database vectors of one workgroup, a wave per pair

BowVector = Tuple[np.ndarray, np.ndarray]


def _vector(v: BowVector):
    return np.ascontiguousarray(v[0], np.uint32).reshape(-1), np.ascontiguousarray(v[1], np.float64).reshape(-1)


def _csr(vs: Sequence[BowVector]):
    vs = [_vector(v) for v in vs]
    p = np.zeros(len(vs) + 1, np.int32)
    for i, (ids, _) in enumerate(vs):
        p[i + 1] = p[i] + len(ids)
    ids = np.ascontiguousarray(np.concatenate([v[0] for v in vs]) if vs else np.zeros(0, np.uint32))
    vals = np.ascontiguousarray(np.concatenate([v[1] for v in vs]) if vs else np.zeros(0, np.float64))
    return p, ids, vals


def pair(scoring: int, a: BowVector, b: BowVector) -> float:
    """orbx_score_pair: the score of (ids ascending, values) `a` against `b` under `scoring`, on the host; needs no handle.  NaN for a
    scoring outside 0 .. 5."""
    (ia, va), (ib, vb) = _vector(a), _vector(b)
    assert len(ia) == len(va) and len(ib) == len(vb)
    return float(_lib.score_lib().orbx_score_pair(int(scoring), ptr(ia), ptr(va), len(ia), ptr(ib), ptr(vb), len(ib)))


class ScoreBatch(_lib.SideHandle):
    """Score matrices of two batches of BowVectors under any scoring but KL; one handle holds one stream on one GPU."""

    def __init__(self, device: int = 0):
        self._S = _lib.score_lib()
        self.device_id = int(device)
        super().__init__(self._S, "orbx_score", int(device))

    pair = staticmethod(pair)

    def matrix(self, scoring: int, q: Sequence[BowVector], db: Sequence[BowVector]) -> np.ndarray:
        """orbx_score_matrix: every (query, database) pair of two lists of (ids, values): [len(q), len(db)] float64."""
        qp, qi, qv = _csr(q)
        dp, di, dv = _csr(db)
        out = np.zeros((len(q), len(db)), np.float64)
        self._check(self._S.orbx_score_matrix(self._h, int(scoring), ptr(qp), ptr(qi), ptr(qv), len(q), ptr(dp), ptr(di), ptr(dv), len(db),
                                              ptr(out)))
        return out

    def matrix_device(self, scoring: int, q_ids, q_vals, q_n, nq: int, q_stride: int, db_ids, db_vals, db_n, ndb: int, db_stride: int,
                      scores=None, stream: int = 0):
        """orbx_score_matrix_device on torch tensors or raw HBM addresses in the fixed-stride layout of BowBatch.transform_device; returns
        the [nq, ndb] float64 score tensor (allocated with torch when `scores` is None).  Asynchronous on `stream` (0: the handle's own)."""
        if scores is None:
            import torch
            dev = q_ids.device if hasattr(q_ids, "device") else torch.device("cuda", self.device_id)
            scores = torch.empty((nq, ndb), dtype=torch.float64, device=dev)
        self._check(self._S.orbx_score_matrix_device(self._h, int(scoring), ptr(addr(q_ids)), ptr(addr(q_vals)), ptr(addr(q_n)), int(nq),
                                                     int(q_stride), ptr(addr(db_ids)), ptr(addr(db_vals)), ptr(addr(db_n)), int(ndb),
                                                     int(db_stride), ptr(addr(scores)), ptr(int(stream))))
        return scores
