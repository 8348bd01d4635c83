/* orbx_fisheye.h — the batched two-camera rig front-end: Frame::ComputeStereoFishEyeMatches (src/Frame.cc:1126-1166) for B fisheye pairs at
 * once, on the descriptors two batch extractions left in HBM.  Not part of the drop-in boundary (include/orbx.h): these entry points live in
 * liborbx_fisheye.so, which links liborbx.so.
 *
 * In scope is what is a pure function of the two frames' descriptors and counts and of a depth per accepted match:
 *   :1144        cv::BFMatcher(NORM_HAMMING).knnMatch(k = 2) of each frame's left lapping rows [monoLeft, Nleft) against its right lapping
 *                rows [monoRight, Nright): per query the two smallest (distance, train index) keys, ties to the lower train index
 *   :1150-1151   Lowe's ratio test, (float)d0 < (float)d1 * 0.7 evaluated as the reference's expression is: the float operand times the
 *                double literal, compared in double, one rounding per operation; the accepted matches in the reference's iteration order
 *                (ascending left row), descMatches of them
 *   :1134-1137, :1157-1163   mvLeftToRightMatch / mvRightToLeftMatch / mvDepth: -1 everywhere, then every accepted pair whose depth is
 *                > 0.0001f (a NaN fails) in pair order, so that of several left rows that chose one right row the last one stays
 * Out of scope is KannalaBrandt8::TriangulateMatches (:1156, camera-model geometry): the caller triangulates the pairs of
 * orbx_fisheye_match_batch_device and hands one depth per pair to orbx_fisheye_finish_batch_device.
 *
 * A handle holds scratch memory, one stream and events of its own; calls on one handle run one after the other (each waits, on the device,
 * for the previous one).  The match and finish forms read no context and change none.  orbx_fisheye_extract_batch_device re-runs both contexts'
 * batch extractions, as orbx_extract_batch_device would, and leaves the contexts exactly as those calls leave them.  A context never holds
 * memory of the handle, so the handle may be destroyed before the contexts.  The device forms make a fixed number of launches whatever the
 * counts are and never synchronise with the host.
 * ORBX_FISHEYE_TILE (1 .. 512: train rows per LDS tile) in the environment at orbx_fisheye_create selects a smaller tile; results do not change.
 *
 * A frame's status, wherever a per-frame count is reported (d_npairs, d_nmatches):
 *   -1  the left or the right count is -1 (orbx_extract_batch_device's mark of a frame whose quadtree overflowed)
 *   -2  the frame is malformed: a count outside 0 .. capacity or a monoIndex outside 0 .. count (checked on the device before anything is
 *       addressed), and in the finish form a pair outside the counts, pairs that do not ascend in `left`, or more pairs than capL
 * Such a frame's outputs are all "nothing" (-1 / 256 / -1.0f); no other frame is affected. */
#ifndef ORBX_FISHEYE_H
#define ORBX_FISHEYE_H

#include <stddef.h>
#include <stdint.h>

#include "orbx.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#define ORBX_FISHEYE_EXPORT __attribute__((visibility("default")))
#else
#define ORBX_FISHEYE_EXPORT
#endif

typedef struct orbx_fisheye orbx_fisheye;
typedef struct orbx_fisheye_pair { int32_t left, right; } orbx_fisheye_pair;   /* absolute rows of the two frames */

/* A two-camera rig: two distinct product contexts on ONE device with identical extractor parameters (nfeatures, levels, scale factor, FAST
 * thresholds and the five result-changing options of the CPU profile), as in Frame's rig constructor.  ORBX_E_INVALID otherwise
 * (reason: orbx_fisheye_last_error(NULL)). */
ORBX_FISHEYE_EXPORT int orbx_fisheye_create(orbx_fisheye** out, orbx_ctx* left, orbx_ctx* right);
ORBX_FISHEYE_EXPORT void orbx_fisheye_destroy(orbx_fisheye* h);
/* The reason of the handle's last failure; with h = NULL the calling thread's last orbx_fisheye_create failure. */
ORBX_FISHEYE_EXPORT const char* orbx_fisheye_last_error(const orbx_fisheye* h);

/* :1144-1151 for nframes frames.  d_descL / d_countsL: [nframes][capL][32] / [nframes][2] = {n, monoIndex} as orbx_extract_batch_device wrote
 * them (16-byte aligned), the right side alike with capR; 1 <= capL, capR <= 2^22.  Frame f's queries are its left rows
 * [countsL[f][1], countsL[f][0]), its train rows its right rows [countsR[f][1], countsR[f][0]); either range may be empty (0 pairs).
 * d_knn_idx / d_knn_dist: [nframes][capL][2] int32, indexed by the ABSOLUTE left row; the indices are ABSOLUTE right rows; a missing neighbour
 *   is -1 / 256, as orbx_knn2_allpairs defines it, and so is every row outside the query range.
 * d_pairs: [nframes][capL]: the accepted matches of frame f in ascending left row, {-1, -1} behind them; d_npairs: [nframes] their number
 *   (descMatches), or the frame's status.
 * Asynchronous on `stream` (NULL: the handle's own). */
ORBX_FISHEYE_EXPORT int orbx_fisheye_match_batch_device(orbx_fisheye* h, int nframes, int capL, int capR, const uint8_t* d_descL,
                                                        const int32_t* d_countsL, const uint8_t* d_descR, const int32_t* d_countsR,
                                                        int32_t* d_knn_idx, int32_t* d_knn_dist, orbx_fisheye_pair* d_pairs, int32_t* d_npairs,
                                                        void* stream);

/* :1134-1137 and :1157-1163.  d_pairs / d_npairs as the call above wrote them (pairs strictly ascending in `left`); d_pair_depth:
 * [nframes][capL] float, the caller's TriangulateMatches value of each pair.
 * d_l2r / d_depth: [nframes][capL], d_r2l: [nframes][capR]: -1 / -1.0f in every slot, then for every pair with depth > 0.0001f
 *   l2r[left] = right, depth[left] = its depth, r2l[right] = left — where several pairs name one right row, the largest left row (the last in
 *   pair order) stays.  d_nmatches: [nframes] the number of those pairs (nMatches), or the frame's status (a negative d_npairs is handed on).
 * The result does not depend on scheduling.  Asynchronous on `stream` (NULL: the handle's own). */
ORBX_FISHEYE_EXPORT int orbx_fisheye_finish_batch_device(orbx_fisheye* h, int nframes, int capL, int capR, const orbx_fisheye_pair* d_pairs,
                                                         const int32_t* d_npairs, const float* d_pair_depth, const int32_t* d_countsL,
                                                         const int32_t* d_countsR, int32_t* d_l2r, int32_t* d_r2l, float* d_depth,
                                                         int32_t* d_nmatches, void* stream);

/* Both extractions and the association in one call: orbx_extract_batch_device of the left frames on `stream` with the lapping area
 * (lapL0, lapL1), of the right frames on the right context's own stream (forked from and joined back into `stream` by events) with
 * (lapR0, lapR1), then orbx_fisheye_match_batch_device with capL = capR = orbx_keypoint_capacity(left).  Both sides share the frame layout
 * (row r of frame f at d_imgs + f*frame_stride + r*row_stride); d_kps* / d_desc* / d_counts* as orbx_extract_batch_device lays them out.
 * Asynchronous on `stream` (NULL: the left context's own stream). */
ORBX_FISHEYE_EXPORT int orbx_fisheye_extract_batch_device(orbx_fisheye* h, const uint8_t* d_imgsL, const uint8_t* d_imgsR, int nframes, int rows,
                                                          int cols, size_t row_stride, size_t frame_stride, int lapL0, int lapL1, int lapR0,
                                                          int lapR1, orbx_keypoint* d_kpsL, uint8_t* d_descL, int32_t* d_countsL,
                                                          orbx_keypoint* d_kpsR, uint8_t* d_descR, int32_t* d_countsR, int32_t* d_knn_idx,
                                                          int32_t* d_knn_dist, orbx_fisheye_pair* d_pairs, int32_t* d_npairs, void* stream);

/* Host-buffer conveniences: arrays of the same layouts in host memory are uploaded, the device form runs on the handle's stream and the
 * results are read back; they return when the results are in the caller's buffers. */
ORBX_FISHEYE_EXPORT int orbx_fisheye_match_batch(orbx_fisheye* h, int nframes, int capL, int capR, const uint8_t* descL, const int32_t* countsL,
                                                 const uint8_t* descR, const int32_t* countsR, int32_t* knn_idx, int32_t* knn_dist,
                                                 orbx_fisheye_pair* pairs, int32_t* npairs);
ORBX_FISHEYE_EXPORT int orbx_fisheye_finish_batch(orbx_fisheye* h, int nframes, int capL, int capR, const orbx_fisheye_pair* pairs,
                                                  const int32_t* npairs, const float* pair_depth, const int32_t* countsL, const int32_t* countsR,
                                                  int32_t* l2r, int32_t* r2l, float* depth, int32_t* nmatches);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_FISHEYE_H */
