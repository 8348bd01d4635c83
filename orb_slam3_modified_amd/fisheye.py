"""The batched two-camera rig front-end over liborbx_fisheye.so (include/orbx_fisheye.h): Frame::ComputeStereoFishEyeMatches
(src/Frame.cc:1126-1166) for B fisheye pairs at once -- the 2-NN of each frame's left lapping rows among its right lapping rows, Lowe's ratio
test at 0.7, the ordered list of accepted pairs, and, once the caller has triangulated them (KannalaBrandt8::TriangulateMatches is camera
geometry and stays with the caller), mvLeftToRightMatch / mvRightToLeftMatch / mvDepth.  All arithmetic runs in the HIP kernels of the library;
this file only marshals buffers."""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import KP_DTYPE, addr, host_array as arr, ptr

TILE = 512                   # train rows per LDS tile (ORBX_FISHEYE_TILE lowers it at create)
QUERIES_PER_WORKGROUP = 256
MAX_CAPACITY = 1 << 22
NO_INDEX, NO_DIST = -1, 256
FRAME_EMPTY, FRAME_MALFORMED = -1, -2
PAIR_DTYPE = np.dtype([("left", "<i4"), ("right", "<i4")])
assert PAIR_DTYPE.itemsize == 8


class FisheyeMatches(NamedTuple):
    """knn_idx / knn_dist [B, capL, 2] (by absolute left row; absolute right rows; -1 / 256 where there is none), pairs [B, capL]
    (PAIR_DTYPE on the host, [B, capL, 2] int32 on the device; {-1, -1} behind the frame's accepted pairs) and npairs [B] (descMatches, or
    -1 / -2: the frame's status)."""
    knn_idx: object
    knn_dist: object
    pairs: object
    npairs: object


class FisheyeStereo(NamedTuple):
    """l2r [B, capL], r2l [B, capR], depth [B, capL] (-1 / -1 / -1.0 where there is no match) and nmatches [B] (nMatches, or the status)."""
    l2r: object
    r2l: object
    depth: object
    nmatches: object


class FisheyeExtraction(NamedTuple):
    """Both sides' keypoints [B, cap], descriptors [B, cap, 32] and counts [B, 2] = {n, monoIndex}, and the association."""
    kpsL: np.ndarray
    descL: np.ndarray
    countsL: np.ndarray
    kpsR: np.ndarray
    descR: np.ndarray
    countsR: np.ndarray
    matches: FisheyeMatches


class FisheyeBatch(_lib.SideHandle):
    """A two-camera rig of two ORBextractor instances with identical parameters on one device."""

    def __init__(self, left_ex, right_ex):
        self._F = _lib.fisheye_lib()
        super().__init__(self._F, "orbx_fisheye", left_ex._ctx, right_ex._ctx)
        self.left, self.right = left_ex, right_ex
        self.capacity = left_ex.capacity
        self._frames = None

    def close(self):
        super().close()
        self._frames = None

    # ---- host arrays -----------------------------------------------------------------------------------
    def match(self, descL, countsL, descR, countsR) -> FisheyeMatches:
        """orbx_fisheye_match_batch: descL [B, capL, 32] / descR [B, capR, 32] uint8, counts [B, 2] int32."""
        descL, descR = np.ascontiguousarray(descL, np.uint8), np.ascontiguousarray(descR, np.uint8)
        B, capL, capR = descL.shape[0], descL.shape[1], descR.shape[1]
        assert descL.shape == (B, capL, 32) and descR.shape == (B, capR, 32)
        cL, cR = arr(countsL, np.int32, B, 2), arr(countsR, np.int32, B, 2)
        m = FisheyeMatches(np.zeros((B, capL, 2), np.int32), np.zeros((B, capL, 2), np.int32), np.zeros((B, capL), PAIR_DTYPE), np.zeros(B, np.int32))
        self._check(self._F.orbx_fisheye_match_batch(self._h, B, capL, capR, ptr(descL), ptr(cL), ptr(descR), ptr(cR), ptr(m.knn_idx),
                                                     ptr(m.knn_dist), ptr(m.pairs), ptr(m.npairs)))
        return m

    def finish(self, pairs, npairs, pair_depth, countsL, countsR, capR: Optional[int] = None) -> FisheyeStereo:
        """orbx_fisheye_finish_batch: pairs [B, capL] / npairs [B] as match() returned them, pair_depth [B, capL] float32 (the caller's
        TriangulateMatches value of each pair); capR defaults to capL."""
        pairs = np.ascontiguousarray(pairs, PAIR_DTYPE)
        B, capL = pairs.shape
        capR = capL if capR is None else int(capR)
        s = FisheyeStereo(np.zeros((B, capL), np.int32), np.zeros((B, capR), np.int32), np.zeros((B, capL), np.float32), np.zeros(B, np.int32))
        self._check(self._F.orbx_fisheye_finish_batch(self._h, B, capL, capR, ptr(pairs), ptr(arr(npairs, np.int32, B)),
                                                      ptr(arr(pair_depth, np.float32, B, capL)), ptr(arr(countsL, np.int32, B, 2)),
                                                      ptr(arr(countsR, np.int32, B, 2)), ptr(s.l2r), ptr(s.r2l), ptr(s.depth), ptr(s.nmatches)))
        return s

    def extract(self, imgsL: np.ndarray, imgsR: np.ndarray, lapL: Sequence[int], lapR: Sequence[int]) -> FisheyeExtraction:
        """Host frames [B, rows, cols] uint8 per side (same shape): both extractions with their lapping areas and the association, through
        orbx_fisheye_extract_batch_device on buffers this call allocates (torch); returns when the results are on the host."""
        import torch
        imgsL, imgsR = np.ascontiguousarray(imgsL), np.ascontiguousarray(imgsR)
        assert imgsL.dtype == np.uint8 and imgsL.ndim == 3 and imgsL.shape == imgsR.shape
        B, H, W = imgsL.shape
        cap = self.capacity
        dev = torch.device("cuda", self.left.device_id if self.left.device_id >= 0 else torch.cuda.current_device())
        tL, tR = torch.from_numpy(imgsL).to(dev), torch.from_numpy(imgsR).to(dev)
        z = lambda *shape, dt=torch.uint8: torch.zeros(shape, dtype=dt, device=dev)   # noqa: E731
        kL, dL, cL = z(B, cap, 28), z(B, cap, 32), z(B, 2, dt=torch.int32)
        kR, dR, cR = z(B, cap, 28), z(B, cap, 32), z(B, 2, dt=torch.int32)
        torch.cuda.synchronize(dev)
        m = self.extract_device(tL, tR, lapL, lapR, kL, dL, cL, kR, dR, cR, stream=torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        self._frames = (tL, tR)     # level 0 of both contexts' last batch: it stays alive until the next batch or close()
        h = lambda t: t.cpu().numpy()   # noqa: E731
        return FisheyeExtraction(h(kL).view(KP_DTYPE).reshape(B, cap), h(dL), h(cL), h(kR).view(KP_DTYPE).reshape(B, cap), h(dR), h(cR),
                                 FisheyeMatches(h(m.knn_idx), h(m.knn_dist), h(m.pairs).view(PAIR_DTYPE).reshape(B, cap), h(m.npairs)))

    # ---- torch device tensors --------------------------------------------------------------------------
    @staticmethod
    def _match_outputs(B, cap, like, out: Optional[FisheyeMatches]) -> FisheyeMatches:
        if out is not None:
            return out
        import torch
        z = lambda *shape: torch.empty(shape, dtype=torch.int32, device=like.device)   # noqa: E731
        return FisheyeMatches(z(B, cap, 2), z(B, cap, 2), z(B, cap, 2), z(B))

    def match_device(self, descL, countsL, descR, countsR, out: Optional[FisheyeMatches] = None, stream=None) -> FisheyeMatches:
        """orbx_fisheye_match_batch_device on torch tensors descL [B, capL, 32] / descR [B, capR, 32] uint8 and counts [B, 2] int32;
        asynchronous on `stream` (None or 0: the handle's own).  Without `out` the result tensors are allocated on the inputs' device."""
        B, capL, capR = int(descL.shape[0]), int(descL.shape[1]), int(descR.shape[1])
        m = self._match_outputs(B, capL, descL, out)
        self._check(self._F.orbx_fisheye_match_batch_device(self._h, B, capL, capR, ptr(addr(descL)), ptr(addr(countsL)), ptr(addr(descR)),
                                                            ptr(addr(countsR)), ptr(addr(m.knn_idx)), ptr(addr(m.knn_dist)), ptr(addr(m.pairs)),
                                                            ptr(addr(m.npairs)), ptr(int(stream or 0))))
        return m

    def finish_device(self, pairs, npairs, pair_depth, countsL, countsR, capR: Optional[int] = None, out: Optional[FisheyeStereo] = None,
                      stream=None) -> FisheyeStereo:
        """orbx_fisheye_finish_batch_device on torch tensors: pairs [B, capL, 2] int32, npairs [B] int32, pair_depth [B, capL] float32."""
        import torch
        B, capL = int(pairs.shape[0]), int(pairs.shape[1])
        capR = capL if capR is None else int(capR)
        if out is None:
            z = lambda *shape, dt=torch.int32: torch.empty(shape, dtype=dt, device=pairs.device)   # noqa: E731
            out = FisheyeStereo(z(B, capL), z(B, capR), z(B, capL, dt=torch.float32), z(B))
        self._check(self._F.orbx_fisheye_finish_batch_device(self._h, B, capL, capR, ptr(addr(pairs)), ptr(addr(npairs)), ptr(addr(pair_depth)),
                                                             ptr(addr(countsL)), ptr(addr(countsR)), ptr(addr(out.l2r)), ptr(addr(out.r2l)),
                                                             ptr(addr(out.depth)), ptr(addr(out.nmatches)), ptr(int(stream or 0))))
        return out

    def extract_device(self, imgsL, imgsR, lapL: Sequence[int], lapR: Sequence[int], kpsL, descL, countsL, kpsR, descR, countsR,
                       out: Optional[FisheyeMatches] = None, stream=None) -> FisheyeMatches:
        """orbx_fisheye_extract_batch_device on torch tensors: imgs [B, rows, cols] uint8 (contiguous, one layout for both sides), kps
        [B, cap, 28] uint8, desc [B, cap, 32] uint8, counts [B, 2] int32 per side.  Asynchronous on `stream` (None or 0: the left
        extractor's own); the frames stay alive as long as either extractor's last batch is read."""
        B, H, W = (int(v) for v in imgsL.shape)
        assert tuple(imgsR.shape) == (B, H, W) and imgsL.is_contiguous() and imgsR.is_contiguous()
        m = self._match_outputs(B, self.capacity, descL, out)
        self._check(self._F.orbx_fisheye_extract_batch_device(self._h, ptr(addr(imgsL)), ptr(addr(imgsR)), B, H, W, W, H * W, int(lapL[0]),
                                                              int(lapL[1]), int(lapR[0]), int(lapR[1]), ptr(addr(kpsL)), ptr(addr(descL)),
                                                              ptr(addr(countsL)), ptr(addr(kpsR)), ptr(addr(descR)), ptr(addr(countsR)),
                                                              ptr(addr(m.knn_idx)), ptr(addr(m.knn_dist)), ptr(addr(m.pairs)), ptr(addr(m.npairs)),
                                                              ptr(int(stream or 0))))
        self.left._last_frames = self.right._last_frames = B
        return m
