"""The batched stereo front-end over liborbx_stereo.so (include/orbx_stereo.h): Frame::ComputeStereoMatches (src/Frame.cc:811-981) for B
rectified pairs at once, on the pyramids two extractors left resident, and both extractions + the association in one call.
All arithmetic runs in the HIP kernels of the library; this file only marshals buffers."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Tuple

import numpy as np

from . import _lib
from ._lib import KP_DTYPE, ptr


@dataclass
class StereoResult:
    """Per-side keypoints [B, cap], descriptors [B, cap, 32] and counts [B, 2] = {n, monoIndex} as orbx_extract_batch_device lays them out,
    mvuRight / mvDepth [B, cap] (-1 where no match and past the left count) and kept [B] (matches after the median filter)."""
    kpsL: np.ndarray
    descL: np.ndarray
    countsL: np.ndarray
    kpsR: np.ndarray
    descR: np.ndarray
    countsR: np.ndarray
    u_right: np.ndarray
    depth: np.ndarray
    kept: np.ndarray

    def frame(self, f: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray, int]:
        """(kpsL, descL, kpsR, descR, mvuRight, mvDepth, kept) of frame f, trimmed to the frame's counts."""
        nL, nR = max(int(self.countsL[f, 0]), 0), max(int(self.countsR[f, 0]), 0)
        return (self.kpsL[f, :nL], self.descL[f, :nL], self.kpsR[f, :nR], self.descR[f, :nR], self.u_right[f, :nL], self.depth[f, :nL],
                int(self.kept[f]))


class StereoBatch(_lib.SideHandle):
    """A rectified rig of two ORBextractor instances with identical parameters on one device; mb = baseline, mbf = baseline * fx."""

    def __init__(self, left_ex, right_ex, mb: float, mbf: float):
        self._S = _lib.stereo_lib()
        super().__init__(self._S, "orbx_stereo", left_ex._ctx, right_ex._ctx, float(mb), float(mbf))
        self.left, self.right, self.mb, self.mbf = left_ex, right_ex, float(mb), float(mbf)
        self.capacity = left_ex.capacity

    def extract(self, imgsL: np.ndarray, imgsR: np.ndarray) -> StereoResult:
        """Host frames [B, rows, cols] uint8 per side (same shape): both extractions (lapping (0, 0)) and the association."""
        imgsL, imgsR = np.ascontiguousarray(imgsL), np.ascontiguousarray(imgsR)
        assert imgsL.dtype == np.uint8 and imgsL.ndim == 3 and imgsL.shape == imgsR.shape
        B, H, W = imgsL.shape
        cap = self.capacity
        r = StereoResult(np.zeros((B, cap), KP_DTYPE), np.zeros((B, cap, 32), np.uint8), np.zeros((B, 2), np.int32),
                         np.zeros((B, cap), KP_DTYPE), np.zeros((B, cap, 32), np.uint8), np.zeros((B, 2), np.int32),
                         np.zeros((B, cap), np.float32), np.zeros((B, cap), np.float32), np.zeros(B, np.int32))
        self._check(self._S.orbx_stereo_extract_batch(self._h, ptr(imgsL), ptr(imgsR), B, H, W, imgsL.strides[1], imgsL.strides[0], ptr(r.kpsL),
                                                      ptr(r.descL), ptr(r.countsL), ptr(r.kpsR), ptr(r.descR), ptr(r.countsR), ptr(r.u_right),
                                                      ptr(r.depth), ptr(r.kept)))
        self.left._last_frames = self.right._last_frames = B
        return r

    def extract_device(self, d_imgsL: int, d_imgsR: int, nframes: int, rows: int, cols: int, row_stride: int, frame_stride: int,
                       d_kpsL: int, d_descL: int, d_countsL: int, d_kpsR: int, d_descR: int, d_countsR: int, d_u_right: int, d_depth: int,
                       d_kept: int, stream: int = 0) -> None:
        """orbx_stereo_extract_batch_device: raw HBM addresses (e.g. torch `tensor.data_ptr()`); asynchronous on `stream`."""
        self._check(self._S.orbx_stereo_extract_batch_device(self._h, ptr(d_imgsL), ptr(d_imgsR), nframes, rows, cols, row_stride, frame_stride,
                                                             ptr(d_kpsL), ptr(d_descL), ptr(d_countsL), ptr(d_kpsR), ptr(d_descR), ptr(d_countsR),
                                                             ptr(d_u_right), ptr(d_depth), ptr(d_kept), ptr(stream)))
        self.left._last_frames = self.right._last_frames = nframes

    def match_device(self, nframes: int, d_kpsL: int, d_descL: int, d_countsL: int, d_kpsR: int, d_descR: int, d_countsR: int,
                     d_u_right: int, d_depth: int, d_kept: int, stream: int = 0) -> None:
        """orbx_stereo_match_batch_device after the caller's own two extract_batch_device calls, ordered before it on `stream`."""
        self._check(self._S.orbx_stereo_match_batch_device(self._h, nframes, ptr(d_kpsL), ptr(d_descL), ptr(d_countsL), ptr(d_kpsR), ptr(d_descR),
                                                           ptr(d_countsR), ptr(d_u_right), ptr(d_depth), ptr(d_kept), ptr(stream)))
