/* orbx_projmatch.h — the batched relocalization and Sim3 matchers: the three ORBmatcher::SearchByProjection overloads that project a
 * keyframe's or a candidate's map points into one frame or keyframe,
 *   kind 0  SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, sAlreadyFound, th, ORBdist) (src/ORBmatcher.cc:1889-2010), the call
 *           Tracking::Relocalization makes per surviving candidate keyframe, with (10, 100) and then (3, 64);
 *   kind 1  SearchByProjection(KeyFrame* pKF, Sim3f& Scw, vpPoints, vpMatched, th, ratioHamming) (:427-532) and the same with vpPointsKFs /
 *           vpMatchedKF (:534-646), LoopClosing's calls per loop / merge candidate with (3, 1.5), (5, 1.0) and (8, 1.5),
 * for B (frame, projected points) items at once, on the keypoints and descriptors a batch extraction left in HBM and the points'
 * descriptors in the pool orbx_mpdesc_* fills.  Not part of the drop-in boundary (include/orbx.h): these entry points live in
 * liborbx_projmatch.so.  The library reads plain device arrays only; it takes nothing from a context.
 *
 * In scope: Nleft == -1, from the point where the map points have been projected: the window, the level range of the kind, the taken
 * test, the Hamming best, the acceptance against the item's limit, for kind 0 the rotation histogram with its three maxima, and the
 * frame's updated bindings as indices.  A keyframe and a frame are the same thing here: KeyFrame::GetFeaturesInArea
 * (src/KeyFrame.cc:704-748) is Frame::GetFeaturesInArea without a level filter over the same 64 x 48 grid.
 * Out of scope:
 *   the pose, the camera model, PredictScale and every `continue` before GetFeaturesInArea (:445-486, :553-599, :1904-1934): the caller
 *   folds them into the point's `valid`;
 *   vpMatchedKF[bestIdx] = vpPointsKFs[iMP] (:639): the caller reads it off kp_match, so the two Sim3 overloads are one routine here;
 *   the two-camera block of :1889 (CurrentFrame.Nleft != -1).
 *
 * The specification is the reference's loop.  For item b = {frame, kind, th, max_dist}, the item's points in index order:
 *   1. a point with valid == 0 is skipped.  The caller folds NULL / isBad() / already found, the depth, the image bounds, the distance
 *      invariance and the viewing angle into the flag.
 *   2. radius = th * scale_factors[level] (:489, :602, :1937): float32, rounded once.  The Sim3 overloads' int th converts exactly.
 *   3. candidates.  Kind 0: Frame::GetFeaturesInArea(u, v, radius, level - 1, level + 1) (:1939, src/Frame.cc:657-723); bCheckLevels is
 *      always true here (maxLevel >= 0), and at level 0 the lower test admits every octave.  Kind 1: the unfiltered
 *      KeyFrame::GetFeaturesInArea(u, v, radius) (:491, :604), then in the walk a keypoint with kpLevel < level - 1 || kpLevel > level is
 *      skipped (:509, :622).  Both kinds: the four early returns, the ix-major, iy-minor, ascending-index walk and the strict
 *      fabs(kp - uv) < radius on both axes.  The grid is the frame's 64 x 48 grid, assigned on the device with Frame::PosInGrid's
 *      arithmetic (src/Frame.cc:725-735) from bounds: inv_w = 64.f / (max_x - min_x), cell = round((x - min_x) * inv_w), float32, nothing
 *      contracted, the division rounded to nearest.
 *   4. in the walk (:501-521, :1949-1964): a keypoint that is taken is skipped: taken on entry (kp_taken, :504 / :1952) or bound by an
 *      earlier point of this row.  The best only: strict `<` from 256, so among equal distances the first in walk order wins.
 *   5. accepted iff (float)bestDist <= max_dist (:523, :636, :1966): max_dist is (float)ORBdist for kind 0 and the float32 product
 *      (float)TH_LOW * ratioHamming for kind 1.  A NaN max_dist accepts nothing.  Then kp_match[best] = the point's index, the keypoint
 *      is taken, nmatches++, and for kind 0 under check_orientation one histogram entry (bin, best) with
 *      rot = point.angle - kp[best].angle, + 360.0f when negative, bin = round(rot * (1.0f / 30)), 30 -> 0 (:1973-1980).
 *   6. kind 0 under check_orientation, after the last point (:1988-2007): ComputeThreeMaxima (:2012-2053) over the 30 entry counts,
 *      strict `>` (ties: the first bin wins), (float)max2 < 0.1f * (float)max1 drops the second and third,
 *      (float)max3 < 0.1f * (float)max1 the third; for every entry in another bin kp_match = -2, nmatches--.  Kind 1 has no histogram,
 *      whatever check_orientation says.
 *   7. a keypoint is bound at most once per row (a bound keypoint is taken for every later point), so there is no last-binder rule and
 *      every removed entry is a keypoint of its own.
 * The candidate lists and distances are those of oracle/match_oracle.cpp: mo_window_search_grid with (level - 1, level + 1) resp.
 * (level - 1, level).  The result does not depend on scheduling.
 *
 * Limits: the reference leaves a valid point with a non-finite u or v undefined; here it has no candidate.  A point with no candidate
 * (or none that is free) is never accepted: the reference would index [-1] there for max_dist >= 256.  Coordinates whose cell products
 * leave the range of int are undefined in the reference too; here the conversion saturates.  At most 32 768 keypoints a frame and 16
 * levels, as the device grids of the product.  The reference asserts that a match's bin lies in 0 .. 29 (:1979); angles that give no bin
 * (a NaN, or a difference whose rounded thirtieth falls outside 0 .. 30) leave no histogram entry here, so such a match is never removed.
 *
 * A handle holds scratch memory, one stream and one event of its own; calls on one handle run one after the other on the device.
 * Environment, read at orbx_projmatch_create (results do not change): ORBX_PROJMATCH_LDS = the largest LDS block in bytes a workgroup may
 * hold an item in (0 .. 151552; items that need more are searched in global memory; what is left of it beside the item's arrays is the room
 * for candidate lists, and a row of points whose lists exceed it is processed in runs of points). */
#ifndef ORBX_PROJMATCH_H
#define ORBX_PROJMATCH_H

#include <stddef.h>
#include <stdint.h>

#include "orbx.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#define ORBX_PROJMATCH_EXPORT __attribute__((visibility("default")))
#else
#define ORBX_PROJMATCH_EXPORT
#endif

#define ORBX_PROJMATCH_MAX_LEVELS 16
#define ORBX_PROJMATCH_MAX_CAPACITY 32768

typedef struct orbx_projmatch orbx_projmatch;

/* The frame side: F frames or keyframes at fixed stride, the buffers a batch extraction leaves.  Neither routine has a stereo gate. */
typedef struct orbx_projmatch_side {
  const orbx_keypoint* d_kps;   /* [nframes][capacity]; x, y, octave and angle are read (mvKeysUn) */
  const uint8_t* d_desc;        /* [nframes][capacity][32], 16-byte aligned */
  const int32_t* d_counts;      /* [nframes][2]: {keypoints, -} */
  const float* d_bounds;        /* [nframes][4] = {min_x, min_y, max_x, max_y}: mnMinX, mnMinY, mnMaxX, mnMaxY */
  int nframes, capacity;
} orbx_projmatch_side;

/* One item: the frame (kind 0) or keyframe (kind 1) the points are searched in, the routine (0 = relocalization, :1889; 1 = Sim3, :427 and
 * :534), the call's th and the accept limit as the reference forms it: (float)ORBdist resp. (float)TH_LOW * ratioHamming. */
typedef struct orbx_projmatch_item {
  int32_t frame, kind;
  float th, max_dist;
} orbx_projmatch_item;

/* One projected map point.  u, v: its projection; angle: pKF->mvKeysUn[i].angle, read for kind 0 under check_orientation only; level:
 * nPredictedLevel; point: its descriptor's row in d_pdesc; valid: see step 1. */
typedef struct orbx_projmatch_point {
  float u, v, angle;
  int32_t level, point, valid;
  int32_t pad[2];
} orbx_projmatch_point;

/* ORBX_E_INVALID for out = NULL or device < 0, ORBX_E_DEVICE when the device cannot be opened (reason: orbx_projmatch_last_error(NULL)). */
ORBX_PROJMATCH_EXPORT int orbx_projmatch_create(orbx_projmatch** out, int device);
ORBX_PROJMATCH_EXPORT void orbx_projmatch_destroy(orbx_projmatch* m);
/* The reason of the handle's last failure; with m = NULL the calling thread's last orbx_projmatch_create failure. */
ORBX_PROJMATCH_EXPORT const char* orbx_projmatch_last_error(const orbx_projmatch* m);

/* The search for items [0, nitems):
 *   d_items    [nitems] orbx_projmatch_item; one frame may appear in many items
 *   d_points   [nitems][mcap] orbx_projmatch_point, 16-byte aligned; d_npts [nitems] int32: row b holds npts[b] points
 *   d_pdesc    [npoints][32]: the points' descriptors, 16-byte aligned (the table orbx_mpdesc_select_device writes)
 *   scale_factors [nlevels] float32 in HOST memory (mvScaleFactors), read during the call
 *   check_orientation  the matcher's mbCheckOrientation, for the whole call
 *   d_kp_taken [nitems][capacity] uint8, IN, or NULL for none: nonzero = keypoint i of item b holds a map point before the call
 *              (CurrentFrame.mvpMapPoints[i2] / vpMatched[idx] non-NULL); never written
 *   d_kp_match [nitems][capacity] int32, OUT: -1 untouched, >= 0 the index in row b of the point this call bound to keypoint i, -2 bound
 *              and then set to NULL by the rotation filter (kind 0 only); whole rows are written, -1 beyond the frame's count
 *   d_nmatches [nitems] int32, OUT: what the reference returns
 * d_nmatches[b] = -1 with a kp_match row of -1 for a malformed item: a frame index outside the side, a count outside 0 .. capacity, npts
 * outside 0 .. mcap, a kind outside 0 .. 1, a th that is not finite, or a valid point among the row's first npts whose level lies outside
 * [0, nlevels) or whose `point` lies outside [0, npoints).  All of it is checked on the device before any of these values addresses
 * memory.
 * Asynchronous on `stream`; NULL is the handle's own stream.
 * ORBX_E_INVALID for what the host can check: NULL arguments, sizes < 1, a capacity above 32 768, nlevels outside 1 .. 16, a misaligned
 * d_desc, d_points or d_pdesc, mcap * capacity or nitems * max(mcap, capacity) beyond INT_MAX, buffers on another device than the
 * handle's. */
ORBX_PROJMATCH_EXPORT int orbx_projmatch_search_device(orbx_projmatch* m, const orbx_projmatch_side* side, const orbx_projmatch_item* d_items,
                                                       int nitems, const orbx_projmatch_point* d_points, const int32_t* d_npts, int mcap,
                                                       const uint8_t* d_pdesc, int npoints, const float* scale_factors, int nlevels,
                                                       int check_orientation, const uint8_t* d_kp_taken, int32_t* d_kp_match,
                                                       int32_t* d_nmatches, void* stream);

/* The same on host arrays of the same layout (the d_ members of side, the items, points, descriptors, kp_taken and results are host
 * pointers here): uploads them, searches, and returns when the results are in the caller's buffers. */
ORBX_PROJMATCH_EXPORT int orbx_projmatch_search(orbx_projmatch* m, const orbx_projmatch_side* side, const orbx_projmatch_item* items, int nitems,
                                                const orbx_projmatch_point* points, const int32_t* npts, int mcap, const uint8_t* pdesc,
                                                int npoints, const float* scale_factors, int nlevels, int check_orientation,
                                                const uint8_t* kp_taken, int32_t* kp_match, int32_t* nmatches);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_PROJMATCH_H */
