"""The batched bag of words over liborbx_bow.so (include/orbx_bow.h): TemplatedVocabulary::transform (TemplatedVocabulary.h:1127-1194) for B
frames at once on descriptors resident in HBM (a batch extraction's buffers, a replay block, a gathered part), and L1Scoring::score for every
pair of two batches.  All arithmetic runs in the HIP kernels of the library; this file only marshals buffers."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import addr, ptr

BowVector = Tuple[np.ndarray, np.ndarray]
FeatureVector = Dict[int, List[int]]


@dataclass
class BowDeviceResult:
    """The fixed-stride device layout of orbx_bow_transform_batch_device as torch tensors: bow_ids / bow_vals [B, cap], bow_n [B], fv_node
    [B, cap], fv_ptr [B, cap + 1], fv_feat [B, cap], fv_n [B].  Slots past a frame's n are unspecified."""
    bow_ids: object
    bow_vals: object
    bow_n: object
    fv_node: object
    fv_ptr: object
    fv_feat: object
    fv_n: object

    def frames(self, which: Optional[Sequence[int]] = None) -> list:
        """Host copies: per frame ((ids, vals), {node: [features]}) — the shape ORBVocabulary.transform returns —, None for a frame whose
        count was negative.  `which`: frame indices (default all)."""
        bi, bv, bn = self.bow_ids.cpu().numpy().view(np.uint32), self.bow_vals.cpu().numpy(), self.bow_n.cpu().numpy()
        fn, fp, ff, fc = (self.fv_node.cpu().numpy().view(np.uint32), self.fv_ptr.cpu().numpy(), self.fv_feat.cpu().numpy().view(np.uint32),
                          self.fv_n.cpu().numpy())
        out = []
        for f in (range(len(bn)) if which is None else which):
            if bn[f] < 0 or fc[f] < 0:
                out.append(None)
                continue
            k, m = int(bn[f]), int(fc[f])
            fv = {int(fn[f, j]): ff[f, fp[f, j]:fp[f, j + 1]].astype(np.int64).tolist() for j in range(m)}
            out.append(((bi[f, :k].copy(), bv[f, :k].copy()), fv))
        return out


class BowBatch(_lib.SideHandle):
    """BowVectors, FeatureVectors and L1 score matrices for batches of frames with one ORBVocabulary (which must stay alive)."""

    def __init__(self, vocabulary, levelsup: int = 4):
        self._B = _lib.bow_lib()
        self.vocabulary, self.levelsup = vocabulary, int(levelsup)
        super().__init__(self._B, "orbx_bow", vocabulary._voc, int(levelsup))

    # ---- transform ---------------------------------------------------------------------------------------
    def transform(self, desc: np.ndarray, counts: np.ndarray) -> list:
        """Host descriptors [B, cap, 32] uint8 and counts ([B, 2] int32 as the batch extraction writes them, or [B] keypoint counts): per
        frame ((ids ascending, values), {node id: [feature indices]}); a frame with a negative count gives empty vectors."""
        desc = np.ascontiguousarray(desc, np.uint8)
        assert desc.ndim == 3 and desc.shape[2] == 32
        B, cap = desc.shape[:2]
        counts = np.asarray(counts, np.int32)
        if counts.ndim == 1:
            counts = np.stack([counts, np.zeros_like(counts)], axis=1)
        counts = np.ascontiguousarray(counts)
        assert counts.shape == (B, 2)
        nk = B * cap
        bow_ptr, fv_ptr = np.zeros(B + 1, np.int32), np.zeros(B + 1, np.int32)
        bow_ids, bow_vals = np.zeros(nk, np.uint32), np.zeros(nk, np.float64)
        fv_node, fv_feat_ptr, fv_feat = np.zeros(nk, np.uint32), np.zeros(nk + 1, np.int32), np.zeros(nk, np.uint32)
        self._check(self._B.orbx_bow_transform_batch(self._h, ptr(desc), ptr(counts), B, cap, ptr(bow_ptr), ptr(bow_ids), ptr(bow_vals), ptr(fv_ptr),
                                                     ptr(fv_node), ptr(fv_feat_ptr), ptr(fv_feat)))
        out = []
        for f in range(B):
            b0, b1, n0, n1 = bow_ptr[f], bow_ptr[f + 1], fv_ptr[f], fv_ptr[f + 1]
            fv = {int(fv_node[j]): fv_feat[fv_feat_ptr[j]:fv_feat_ptr[j + 1]].astype(np.int64).tolist() for j in range(n0, n1)}
            out.append(((bow_ids[b0:b1].copy(), bow_vals[b0:b1].copy()), fv))
        return out

    def transform_device(self, d_desc, d_counts, nframes: int, capacity: int, out: Optional[BowDeviceResult] = None, stream: int = 0,
                         bow: bool = True, fv: bool = True) -> BowDeviceResult:
        """orbx_bow_transform_batch_device on torch tensors or raw HBM addresses; asynchronous on `stream` (0: the handle's own).  Without
        `out` the result tensors are allocated on d_desc's device (torch).  bow / fv = False skips that output group."""
        if out is None:
            import torch
            dev = d_desc.device if hasattr(d_desc, "device") else torch.device("cuda", 0)
            z = lambda *shape, dt: torch.empty(shape, dtype=dt, device=dev)   # noqa: E731
            out = BowDeviceResult(z(nframes, capacity, dt=torch.int32), z(nframes, capacity, dt=torch.float64), z(nframes, dt=torch.int32),
                                  z(nframes, capacity, dt=torch.int32), z(nframes, capacity + 1, dt=torch.int32),
                                  z(nframes, capacity, dt=torch.int32), z(nframes, dt=torch.int32))
        b = (out.bow_ids, out.bow_vals, out.bow_n) if bow else (None, None, None)
        v = (out.fv_node, out.fv_ptr, out.fv_feat, out.fv_n) if fv else (None, None, None, None)
        self._check(self._B.orbx_bow_transform_batch_device(self._h, ptr(addr(d_desc)), ptr(addr(d_counts)), int(nframes), int(capacity),
                                                            *(ptr(addr(t)) for t in b + v), ptr(int(stream))))
        return out

    # ---- scores ------------------------------------------------------------------------------------------
    @staticmethod
    def _csr(vs: Sequence[BowVector]):
        p = np.zeros(len(vs) + 1, np.int32)
        for i, (ids, _) in enumerate(vs):
            p[i + 1] = p[i] + len(ids)
        ids = np.ascontiguousarray(np.concatenate([np.asarray(v[0], np.uint32) for v in vs]) if len(vs) else np.zeros(0, np.uint32))
        vals = np.ascontiguousarray(np.concatenate([np.asarray(v[1], np.float64) for v in vs]) if len(vs) else np.zeros(0, np.float64))
        return p, ids, vals

    def score_matrix(self, q: Sequence[BowVector], db: Sequence[BowVector]) -> np.ndarray:
        """L1Scoring::score of every (query, database) pair of two lists of (ids, values): [len(q), len(db)] float64."""
        qp, qi, qv = self._csr(q)
        dp, di, dv = self._csr(db)
        out = np.zeros((len(q), len(db)), np.float64)
        self._check(self._B.orbx_bow_score_matrix(self._h, ptr(qp), ptr(qi), ptr(qv), len(q), ptr(dp), ptr(di), ptr(dv), len(db), ptr(out)))
        return out

    def score_matrix_device(self, q_ids, q_vals, q_n, nq: int, q_stride: int, db_ids, db_vals, db_n, ndb: int, db_stride: int, scores=None,
                            stream: int = 0):
        """orbx_bow_score_matrix_device on torch tensors or raw HBM addresses in the fixed-stride layout of transform_device; returns the
        [nq, ndb] float64 score tensor (allocated with torch when `scores` is None).  Asynchronous on `stream`."""
        if scores is None:
            import torch
            dev = q_ids.device if hasattr(q_ids, "device") else torch.device("cuda", 0)
            scores = torch.empty((nq, ndb), dtype=torch.float64, device=dev)
        self._check(self._B.orbx_bow_score_matrix_device(self._h, ptr(addr(q_ids)), ptr(addr(q_vals)), ptr(addr(q_n)), int(nq), int(q_stride),
                                                         ptr(addr(db_ids)), ptr(addr(db_vals)), ptr(addr(db_n)), int(ndb), int(db_stride),
                                                         ptr(addr(scores)), ptr(int(stream))))
        return scores
