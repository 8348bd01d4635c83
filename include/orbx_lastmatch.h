/* orbx_lastmatch.h — the batched frame-to-last-frame matcher: ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th,
 * bMono) (src/ORBmatcher.cc:1676-1885), the call Tracking::TrackWithMotionModel makes on every tracked frame, for B (current frame, last
 * frame's points) items at once, on the keypoints and descriptors a batch extraction left in HBM and the points' descriptors in the pool
 * orbx_mpdesc_* fills.  Not part of the drop-in boundary (include/orbx.h): these entry points live in liborbx_lastmatch.so.  The library
 * reads plain device arrays only; it takes nothing from a context.
 *
 * In scope: CurrentFrame.Nleft == -1, from the point where the last frame's map points have been projected (the cut
 * orbx_search_by_projection_last and the oracle's mo_search_by_projection_last make): the window, the level range of the direction, the
 * stereo gate, the Hamming best, the acceptance, the rotation histogram with its three maxima, and the current frame's updated
 * mvpMapPoints as indices.
 * Out of scope:
 *   the pose and camera-model arithmetic of :1686-1718, bForward / bBackward included: the caller passes them as `direction`;
 *   the two-camera block (:1794-1880): with Nleft != -1 the whole routine is include/orbx_rigmatch.h's (liborbx_rigmatch.so).
 *
 * The specification is the reference's loop.  For item b = {frame, direction, mbf, th}, the item's points in index order:
 *   1. a point with valid == 0 is skipped.  The caller folds `pMP`, !mvbOutlier[i], invzc >= 0 and the image-bounds tests (:1697-1718)
 *      into the flag, as orbx_search_by_projection_last documents.
 *   2. radius = th * scale_factors[octave] (:1724): float32, rounded once.
 *   3. candidates: Frame::GetFeaturesInArea(u, v, radius, minLevel, maxLevel) (src/Frame.cc:657-723) with (octave, -1) for direction 1
 *      (bForward, :1729), (0, octave) for direction 2 (bBackward, :1731) and (octave - 1, octave + 1) otherwise (:1733); its four early
 *      returns, bCheckLevels = minLevel > 0 || maxLevel >= 0, the upper test applied only when maxLevel >= 0, the ix-major, iy-minor,
 *      ascending-index walk and the strict fabs(kp - uv) < radius on both axes.  Hence forward at octave 0 checks no level, backward at
 *      octave 0 admits octave 0 only, neither at octave 0 admits octaves 0 and 1.  The grid is the frame's 64 x 48 grid, assigned on the
 *      device with Frame::PosInGrid's arithmetic (src/Frame.cc:725-735) from bounds: inv_w = 64.f / (max_x - min_x),
 *      cell = round((x - min_x) * inv_w), float32, nothing contracted.
 *   4. in the walk (:1743-1768): a keypoint with kp_obs[i2] > 0 is skipped; on a stereo side, when u_right[i2] > 0,
 *      ur = u - mbf * invz (a float32 product, then a float32 subtraction: never a fused multiply-add), er = fabs(ur - u_right[i2]), and
 *      the keypoint is skipped when er > radius.  The best only: strict `<` from 256, so among equal distances the first in walk order wins.
 *   5. accepted iff bestDist <= 100 (:1770).  Then kp_match[best] = the point's index, kp_obs[best] = the point's obs, nmatches++, and
 *      under check_orientation one histogram entry (bin, best) with rot = point.angle - kp[best].angle, + 360.0f when negative,
 *      bin = round(rot * (1.0f / 30)), 30 -> 0 (:1784-1791).  A point with obs <= 0 does not hide its keypoint: a later point may rebind
 *      it; both bindings count in nmatches and both leave a histogram entry.
 *   6. after the last point, under check_orientation (:1862-1882): ComputeThreeMaxima (:2012-2053) over the 30 entry counts, strict `>`
 *      (ties: the first bin wins), (float)max2 < 0.1f * (float)max1 drops the second and third, (float)max3 < 0.1f * (float)max1 the
 *      third; for every entry in another bin kp_match = -2, kp_obs = -1, nmatches--.  A rebound keypoint with entries in a kept and in a
 *      removed bin ends at -2, and every removed entry decrements nmatches.
 * Bit for bit oracle/match_oracle.cpp: mo_search_by_projection_last.  The result does not depend on scheduling.
 *
 * Limits: the reference leaves a valid point with a non-finite u or v undefined; here it has no candidate.  Coordinates whose cell
 * products leave the range of int are undefined in the reference too; here the conversion saturates.  At most 32 768 keypoints a frame and
 * 16 levels, as the device grids of the product.  The reference asserts that a match's bin lies in 0 .. 29 (:1790); angles that give no
 * bin (a NaN, or a difference whose rounded thirtieth falls outside 0 .. 30) leave no histogram entry here, so such a match is never removed.
 *
 * A handle holds scratch memory, one stream and one event of its own; calls on one handle run one after the other on the device.
 * Environment, read at orbx_lastmatch_create (results do not change): ORBX_LASTMATCH_LDS = the largest LDS block in bytes a workgroup may
 * hold an item in (0 .. 151552; items that need more are searched in global memory; what is left of it beside the item's arrays is the room
 * for candidate lists, and a row of points whose lists exceed it is processed in runs of points). */
#ifndef ORBX_LASTMATCH_H
#define ORBX_LASTMATCH_H

#include <stddef.h>
#include <stdint.h>

#include "orbx.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#define ORBX_LASTMATCH_EXPORT __attribute__((visibility("default")))
#else
#define ORBX_LASTMATCH_EXPORT
#endif

#define ORBX_LASTMATCH_MAX_LEVELS 16
#define ORBX_LASTMATCH_MAX_CAPACITY 32768

typedef struct orbx_lastmatch orbx_lastmatch;

/* The frame side: F current frames at fixed stride, the buffers a batch extraction leaves. */
typedef struct orbx_lastmatch_side {
  const orbx_keypoint* d_kps;   /* [nframes][capacity]; x, y, octave and angle are read (mvKeysUn) */
  const uint8_t* d_desc;        /* [nframes][capacity][32], 16-byte aligned */
  const int32_t* d_counts;      /* [nframes][2]: {keypoints, -} */
  const float* d_uright;        /* [nframes][capacity], or NULL: a monocular side (no stereo gate).  mvuRight: the gate reads uright > 0 */
  const float* d_bounds;        /* [nframes][4] = {min_x, min_y, max_x, max_y}: mnMinX, mnMinY, mnMaxX, mnMaxY */
  int nframes, capacity;
} orbx_lastmatch_side;

/* One item: the current frame it is tracked in, 0 = neither, 1 = bForward, 2 = bBackward (as orbx_search_by_projection_last), the
 * current frame's mbf (read under the stereo gate only) and the call's th (per item: Tracking retries a frame with 2 * th). */
typedef struct orbx_lastmatch_item {
  int32_t frame, direction;
  float mbf, th;
} orbx_lastmatch_item;

/* One point of the last frame.  u, v: its projection into the current frame; invz: invzc; angle: the last frame's keypoint angle; octave:
 * nLastOctave; obs: the map point's Observations(); point: its descriptor's row in d_pdesc. */
typedef struct orbx_lastmatch_point {
  float u, v, invz, angle;
  int32_t octave, obs, point, valid;
} orbx_lastmatch_point;

/* ORBX_E_INVALID for out = NULL or device < 0, ORBX_E_DEVICE when the device cannot be opened (reason: orbx_lastmatch_last_error(NULL)). */
ORBX_LASTMATCH_EXPORT int orbx_lastmatch_create(orbx_lastmatch** out, int device);
ORBX_LASTMATCH_EXPORT void orbx_lastmatch_destroy(orbx_lastmatch* m);
/* The reason of the handle's last failure; with m = NULL the calling thread's last orbx_lastmatch_create failure. */
ORBX_LASTMATCH_EXPORT const char* orbx_lastmatch_last_error(const orbx_lastmatch* m);

/* The search for items [0, nitems):
 *   d_items    [nitems] orbx_lastmatch_item; one current frame may appear in many items
 *   d_points   [nitems][mcap] orbx_lastmatch_point, 16-byte aligned; d_nlast [nitems] int32: row b holds nlast[b] points
 *   d_pdesc    [npoints][32]: the points' descriptors, 16-byte aligned (the table orbx_mpdesc_select_device writes)
 *   scale_factors [nlevels] float32 in HOST memory (mvScaleFactors), read during the call
 *   check_orientation  the matcher's mbCheckOrientation, for the whole call
 *   d_kp_obs   [nitems][capacity] int32, IN / OUT: Observations() of the map point keypoint i of item b holds, -1 without one
 *   d_kp_match [nitems][capacity] int32, OUT: -1 untouched, >= 0 the index in row b of the point this call bound to keypoint i, -2 set to
 *              NULL by the rotation filter; whole rows are written, -1 beyond the frame's count
 *   d_nmatches [nitems] int32, OUT: what the reference returns
 * d_nmatches[b] = -1 with a kp_match row of -1 and an untouched kp_obs row for a malformed item: a frame index outside the side, a count
 * outside 0 .. capacity, nlast outside 0 .. mcap, a direction outside 0 .. 2, a th that is not finite, or a valid point among the row's
 * first nlast whose octave lies outside [0, nlevels) or whose `point` lies outside [0, npoints).  All of it is checked on the device before
 * any of these values addresses memory.
 * Asynchronous on `stream`; NULL is the handle's own stream.
 * ORBX_E_INVALID for what the host can check: NULL arguments, sizes < 1, a capacity above 32 768, nlevels outside 1 .. 16, a misaligned
 * d_desc, d_points or d_pdesc, mcap * capacity or nitems * max(mcap, capacity) beyond INT_MAX, buffers on another device than the
 * handle's. */
ORBX_LASTMATCH_EXPORT int orbx_lastmatch_search_device(orbx_lastmatch* m, const orbx_lastmatch_side* side, const orbx_lastmatch_item* d_items,
                                                       int nitems, const orbx_lastmatch_point* d_points, const int32_t* d_nlast, int mcap,
                                                       const uint8_t* d_pdesc, int npoints, const float* scale_factors, int nlevels,
                                                       int check_orientation, int32_t* d_kp_obs, int32_t* d_kp_match, int32_t* d_nmatches,
                                                       void* stream);

/* The same on host arrays of the same layout (the d_ members of side, the items, points, descriptors and results are host pointers here):
 * uploads them, searches, and returns when the results are in the caller's buffers; kp_obs is read and updated. */
ORBX_LASTMATCH_EXPORT int orbx_lastmatch_search(orbx_lastmatch* m, const orbx_lastmatch_side* side, const orbx_lastmatch_item* items, int nitems,
                                                const orbx_lastmatch_point* points, const int32_t* nlast, int mcap, const uint8_t* pdesc,
                                                int npoints, const float* scale_factors, int nlevels, int check_orientation, int32_t* kp_obs,
                                                int32_t* kp_match, int32_t* nmatches);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_LASTMATCH_H */
