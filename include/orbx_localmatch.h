/* orbx_localmatch.h — the batched SearchLocalPoints: ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th, ...)
 * (src/ORBmatcher.cc:43-141), the call Tracking::SearchLocalPoints makes on every tracked frame, for B (frame, local map) items at once, on
 * the keypoints and descriptors a batch extraction left in HBM and the map points' descriptors in the pool orbx_mpdesc_* fills.  Not part of
 * the drop-in boundary (include/orbx.h): these entry points live in liborbx_localmatch.so.  The library reads plain device arrays only; it
 * takes nothing from a context.
 *
 * In scope: F.Nleft == -1, from the point where every map point carries mTrackProjX / mTrackProjY / mTrackProjXR, mTrackViewCos and
 * mnTrackScaleLevel: the window, the level range, the stereo gate, the Hamming best / second, the acceptance and the frame's updated
 * mvpMapPoints as indices.
 * Out of scope:
 *   the two-camera block (:143-210): with Nleft != -1 the whole routine is include/orbx_rigmatch.h's (liborbx_rigmatch.so);
 *   the projection that produces those members (Frame::isInFrustum): the caller's Eigen and libm work;
 *   SearchByProjection(Frame, LastFrame) (:1676): the frame-to-last-frame form is include/orbx_lastmatch.h's (liborbx_lastmatch.so).
 *
 * The specification is the reference's loop.  For item b, frame f = frames[b], the item's map points in index order:
 *   1. a point with in_view == 0 is skipped.  The caller folds !mbTrackInView, isBad() and the far-point test into the flag, as
 *      orbx_search_by_projection documents.
 *   2. r = ((double)view_cos > 0.998) ? 2.5f : 4.0f (float against the double literal: float32(0.998) is above it and gives 2.5); when
 *      (double)th != 1.0, r *= th; radius = r * scale_factors[level]: float32, every operation rounded once.
 *   3. candidates: Frame::GetFeaturesInArea(proj_x, proj_y, radius, level - 1, level) (src/Frame.cc:657-723) with its four early returns,
 *      bCheckLevels = minLevel > 0 || maxLevel >= 0 (level 0 passes minLevel = -1), the ix-major, iy-minor, ascending-index walk and the
 *      strict fabs(kp - proj) < radius on both axes.  The grid is the frame's 64 x 48 grid, assigned on the device with Frame::PosInGrid's
 *      arithmetic (src/Frame.cc:725-735) from bounds: inv_w = 64.f / (max_x - min_x), cell = round((x - min_x) * inv_w), float32, nothing
 *      contracted.
 *   4. in the walk: a keypoint with kp_obs[idx] > 0 is skipped; on a stereo side, when u_right[idx] > 0, it is skipped when
 *      fabs(proj_xr - u_right[idx]) > radius.  best / second with strict `<` and `else if (dist < bestDist2)`, both from 256 and level -1;
 *      bestLevel and bestLevel2 are the octaves of the holders: the two smallest (distance, walk position) of the surviving candidates.
 *   5. accepted iff bestDist <= 100 and (bestLevel != bestLevel2 || (float)bestDist <= nn_ratio * (float)bestDist2).
 *   6. on acceptance kp_match[bestIdx] = the point's index, kp_obs[bestIdx] = the point's obs, nmatches++.  A point with obs == 0 does not
 *      hide its keypoint: a later point may rebind it; the later one stands in kp_match and both count in nmatches.
 * Bit for bit oracle/match_oracle.cpp: mo_search_by_projection.  The result does not depend on scheduling.
 *
 * Limits: the reference leaves an in-view point with a non-finite proj_x, proj_y or view_cos undefined; here it has no candidate.
 * Coordinates whose cell products leave the range of int are undefined in the reference too; here the conversion saturates.  At most 32 768
 * keypoints a frame and 16 levels, as the device grids of the product; a candidate's octave is compared in 5 bits (-1 .. 15: what the level
 * range lets through).
 *
 * A handle holds scratch memory, one stream and one event of its own; calls on one handle run one after the other on the device.
 * Environment, read at orbx_localmatch_create (results do not change): ORBX_LOCALMATCH_LDS = the largest LDS block in bytes a workgroup may
 * hold an item in (0 .. 151552; items that need more are searched in global memory; what is left of it beside the item's arrays is the room
 * for candidate lists, and a local map whose lists exceed it is processed in runs of points). */
#ifndef ORBX_LOCALMATCH_H
#define ORBX_LOCALMATCH_H

#include <stddef.h>
#include <stdint.h>

#include "orbx.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#define ORBX_LOCALMATCH_EXPORT __attribute__((visibility("default")))
#else
#define ORBX_LOCALMATCH_EXPORT
#endif

#define ORBX_LOCALMATCH_MAX_LEVELS 16
#define ORBX_LOCALMATCH_MAX_CAPACITY 32768

typedef struct orbx_localmatch orbx_localmatch;

/* The frame side: F frames at fixed stride, the buffers a batch extraction leaves. */
typedef struct orbx_localmatch_side {
  const orbx_keypoint* d_kps;   /* [nframes][capacity]; x, y and octave are read (mvKeysUn) */
  const uint8_t* d_desc;        /* [nframes][capacity][32], 16-byte aligned */
  const int32_t* d_counts;      /* [nframes][2]: {keypoints, -} */
  const float* d_uright;        /* [nframes][capacity], or NULL: a monocular side (no stereo gate).  mvuRight: the gate reads uright > 0 */
  const float* d_bounds;        /* [nframes][4] = {min_x, min_y, max_x, max_y}: mnMinX, mnMinY, mnMaxX, mnMaxY */
  int nframes, capacity;
} orbx_localmatch_side;

/* One map point of an item's local map.  point: its descriptor's row in d_pdesc.  proj_xr is read under the stereo gate only. */
typedef struct orbx_localmatch_point {
  float proj_x, proj_y, proj_xr, view_cos;
  int32_t level, obs, point, in_view;
} orbx_localmatch_point;

/* ORBX_E_INVALID for out = NULL or device < 0, ORBX_E_DEVICE when the device cannot be opened (reason: orbx_localmatch_last_error(NULL)). */
ORBX_LOCALMATCH_EXPORT int orbx_localmatch_create(orbx_localmatch** out, int device);
ORBX_LOCALMATCH_EXPORT void orbx_localmatch_destroy(orbx_localmatch* m);
/* The reason of the handle's last failure; with m = NULL the calling thread's last orbx_localmatch_create failure. */
ORBX_LOCALMATCH_EXPORT const char* orbx_localmatch_last_error(const orbx_localmatch* m);

/* The search for items [0, nitems):
 *   d_frames   [nitems] int32: the frame item b is tracked in; one frame may appear in many items
 *   d_mp       [nitems][mcap] orbx_localmatch_point, 16-byte aligned; d_nmp [nitems] int32: row b holds nmp[b] points
 *   d_pdesc    [npoints][32]: the map points' descriptors, 16-byte aligned (the table orbx_mpdesc_select_device writes)
 *   scale_factors [nlevels] float32 in HOST memory (mvScaleFactors), read during the call
 *   th, nn_ratio  the call's th and the matcher's mfNNratio
 *   d_kp_obs   [nitems][capacity] int32, IN / OUT: Observations() of the map point keypoint i of item b holds, -1 without one
 *   d_kp_match [nitems][capacity] int32, OUT: the index in row b of the point this call bound to keypoint i, -1 untouched; whole rows
 *              are written, -1 beyond the frame's count
 *   d_nmatches [nitems] int32, OUT: what the reference returns
 * d_nmatches[b] = -1 with a kp_match row of -1 and an untouched kp_obs row for a malformed item: a frame index outside the side, a count
 * outside 0 .. capacity, nmp outside 0 .. mcap, or an in-view point among the row's first nmp whose level lies outside [0, nlevels) or
 * whose `point` lies outside [0, npoints).  All of it is checked on the device before any of these values addresses memory.
 * Asynchronous on `stream`; NULL is the handle's own stream.
 * ORBX_E_INVALID for what the host can check: NULL arguments, sizes < 1, a capacity above 32 768, nlevels outside 1 .. 16, a th that is not
 * finite, a misaligned d_desc, d_mp or d_pdesc, mcap * capacity or nitems * max(mcap, capacity) beyond INT_MAX, buffers on another device
 * than the handle's. */
ORBX_LOCALMATCH_EXPORT int orbx_localmatch_search_device(orbx_localmatch* m, const orbx_localmatch_side* side, const int32_t* d_frames,
                                                         int nitems, const orbx_localmatch_point* d_mp, const int32_t* d_nmp, int mcap,
                                                         const uint8_t* d_pdesc, int npoints, const float* scale_factors, int nlevels, float th,
                                                         float nn_ratio, int32_t* d_kp_obs, int32_t* d_kp_match, int32_t* d_nmatches,
                                                         void* stream);

/* The same on host arrays of the same layout (the d_ members of side, the items, descriptors and results are host pointers here): uploads
 * them, searches, and returns when the results are in the caller's buffers; kp_obs is read and updated. */
ORBX_LOCALMATCH_EXPORT int orbx_localmatch_search(orbx_localmatch* m, const orbx_localmatch_side* side, const int32_t* frames, int nitems,
                                                  const orbx_localmatch_point* mp, const int32_t* nmp, int mcap, const uint8_t* pdesc,
                                                  int npoints, const float* scale_factors, int nlevels, float th, float nn_ratio,
                                                  int32_t* kp_obs, int32_t* kp_match, int32_t* nmatches);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_LOCALMATCH_H */
