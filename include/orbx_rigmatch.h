/* orbx_rigmatch.h — the two-camera rig blocks of Tracking's two projection matchers, batched: ORBmatcher::SearchByProjection(Frame&, const
 * vector<MapPoint*>&, th, ...) (src/ORBmatcher.cc:43-212, SearchLocalPoints) and ORBmatcher::SearchByProjection(Frame& CurrentFrame, const
 * Frame& LastFrame, th, bMono) (:1676-1886), both with Nleft != -1, for B items at once on the buffers a batched rig extraction
 * (include/orbx_fisheye.h) left in HBM: a left and a right extraction and mvLeftToRightMatch / mvRightToLeftMatch.  Not part of the drop-in
 * boundary (include/orbx.h): these entry points live in liborbx_rigmatch.so.  The library reads plain device arrays only; it takes nothing
 * from a context.  The Nleft == -1 forms are include/orbx_localmatch.h's and include/orbx_lastmatch.h's.
 *
 * The rig block of SearchByBoW (:296-323, :357-386) and the stacked rig frame it needs are include/orbx_rigbow.h's (liborbx_rigbow.so).
 * Out of scope: the rig blocks of the relocalization SearchByProjection (:1889), of Fuse (bRight) and of SearchForTriangulation;
 * the KannalaBrandt8 projections that produce the rows (Frame::isInFrustum's two-camera part, Trl * x3Dc at :1795-1796): the caller's.
 *
 * The rig side.  Two frame sides in orbx_localmatch_side's layout with capacities of their own, cap_l and cap_r; the keypoints are the RAW
 * mvKeys / mvKeysRight (the reference reads no mvKeysUn when Nleft != -1).  ONE d_bounds row per frame: both grids use the frame's
 * mnMinX .. mnMaxY and the same Frame::PosInGrid arithmetic (src/Frame.cc:385-416, :657-723 with bRight).  d_l2r / d_r2l as
 * orbx_fisheye_finish_batch_device writes them.  No u_right: the stereo gate is off for rigs (:92, :1751).
 * Slots.  d_kp_obs (IN / OUT) and d_kp_match (OUT) are rows of cap_l + cap_r per item: slot i < cap_l is left keypoint i, slot cap_l + j is
 * right keypoint j (the reference's j + Nleft at a fixed stride).
 * Limits: cap_l + cap_r <= 32 768 (indices stay 15-bit, the hidden bits 4 KiB), at most 16 levels.  A non-finite projection has no
 * candidate.  Coordinates whose cell products leave the range of int saturate.
 *
 * Entry 1, orbx_rigmatch_local: :43-212.  A slot is HIDDEN when its current holder has Observations() > 0 (kp_obs[slot] > 0).  For item b,
 * frame f = frames[b], the item's points in index order:
 *   1. a point with neither in_view nor in_view_r is skipped.  The caller folds isBad() and the far-point test into BOTH flags: they skip
 *      the whole point.
 *   2. the left block, if in_view: r = ((double)view_cos > 0.998) ? 2.5f : 4.0f; when (double)th != 1.0, r *= th; radius = r * sf[level];
 *      Frame::GetFeaturesInArea(proj_x, proj_y, radius, level - 1, level) over the LEFT grid (the window of orbx_localmatch.h step 3);
 *      candidates whose slot is hidden are passed over; best / second with strict `<` and `else if (dist < bestDist2)`, both from 256 and
 *      level -1, and their octaves.  An empty list or bestDist > 100 falls through to the right block.  When bestDist <= 100, the two
 *      octaves are equal and (float)bestDist > nn_ratio * (float)bestDist2, the point is DONE: the `continue` of :126 skips its right block
 *      too.  Otherwise (the octaves differ, or (float)bestDist <= nn_ratio * (float)bestDist2) it is accepted: kp_match[best] = q,
 *      kp_obs[best] = obs, nmatches++; and when l2r[best] != -1 also kp_match[cap_l + l2r[best]] = q with its kp_obs and nmatches++ again
 *      (:131-135).  That binding is unconditional: it overwrites whatever the slot held, hidden or not.
 *   3. the right block, if in_view_r and level_r != -1: r from view_cos_r, NOT multiplied by th (:147); radius = r * sf[level_r];
 *      the window (proj_xr, proj_yr, radius, level_r - 1, level_r) over the RIGHT grid; the hidden test is on slot cap_l + idx and sees
 *      what step 2 of this same point bound; best / second on the right octaves.  When bestDist <= 100 and not (equal octaves and
 *      (float)bestDist > nn_ratio * (float)bestDist2): when r2l[best] != -1, kp_match[r2l[best]] = q with kp_obs and nmatches++ (:198-202,
 *      unconditional too); then kp_match[cap_l + best] = q, kp_obs, nmatches++.
 * Two consequences the one-camera kernel does not have: a write by a point with obs <= 0 CLEARS a slot's hidden state (a cross-binding, or
 * the rebinding of an open slot), so the hidden state is set or cleared on every write by the writer's obs; and a slot's final holder is
 * its LAST writer: the points run in index order, so kp_match[slot] is the largest index among its writers and kp_obs[slot] that point's
 * obs.
 *
 * Entry 2, orbx_rigmatch_last: :1676-1886.  The caller projects both cameras and folds pMP, the outlier flag, invzc < 0 and the LEFT image
 * bounds tests into `valid` (each skips both blocks); the right projection is not bounds-tested by the reference.  mbf is unused for rigs.
 * For every valid point of the item in index order:
 *   1. the left block: radius = th * sf[octave]; the window (u, v, radius) over the left grid with the direction's level range: direction
 *      1 (bForward) (octave, -1), 2 (bBackward) (0, octave), 0 (octave - 1, octave + 1).  An EMPTY list ends the point (:1735): its right
 *      block is not run.  Hidden candidates are passed over; best only, strict `<`.  When bestDist <= 100: kp_match[best] = q, kp_obs,
 *      nmatches++ and a histogram entry from angle - the LEFT keypoint's angle on slot `best`.  There is no l2r binding in this routine.
 *   2. the right block, whenever step 1's list was not empty, accepted or not: the same radius, the window (u_r, v_r, radius) over the
 *      right grid with the same level ranges (:1806-1811); the hidden test on cap_l + i2; when bestDist <= 100: kp_match[cap_l + best] = q,
 *      kp_obs, nmatches++ and a histogram entry from the RIGHT keypoint's angle on slot cap_l + best.
 *   3. after the last point, under check_orientation: ComputeThreeMaxima (:2012-2053) over all entries (a point may leave two); every
 *      entry of another bin sets kp_match[slot] = -2 and kp_obs[slot] = -1 and decrements nmatches.
 *
 * Both entries, a malformed item: nmatches = -1, a kp_match row of -1 and an untouched kp_obs row.  Malformed: a frame index outside the
 * side; a left or right count outside 0 .. its capacity; the row's count outside 0 .. mcap; among the row's first points an in-view
 * (valid) one whose level (octave) lies outside [0, nlevels) -- for the right side of entry 1 level_r == -1 is allowed too -- or whose
 * `point` lies outside the pool; for entry 1 an l2r entry below the left count outside [-1, right count) or an r2l entry below the right
 * count outside [-1, left count); for entry 2 a direction outside 0 .. 2 or a th that is not finite.  All of it is checked on the device
 * before any of these values addresses memory.  The results do not depend on scheduling.
 *
 * A handle holds scratch memory, one stream and one event of its own; calls on one handle run one after the other on the device.
 * Environment, read at orbx_rigmatch_create (results do not change): ORBX_RIGMATCH_LDS = the largest LDS block in bytes a workgroup may hold
 * an item in (0 .. 151552; items that need more are searched in global memory; what is left of it beside the item's arrays is the room for
 * candidate lists, and a row whose lists exceed it is processed in runs of points). */
#ifndef ORBX_RIGMATCH_H
#define ORBX_RIGMATCH_H

#include <stddef.h>
#include <stdint.h>

#include "orbx.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#define ORBX_RIGMATCH_EXPORT __attribute__((visibility("default")))
#else
#define ORBX_RIGMATCH_EXPORT
#endif

#define ORBX_RIGMATCH_MAX_LEVELS 16
#define ORBX_RIGMATCH_MAX_CAPACITY 32768   /* cap_l + cap_r */

typedef struct orbx_rigmatch orbx_rigmatch;

/* The rig side: F frames at fixed strides, the buffers a batched rig extraction leaves. */
typedef struct orbx_rigmatch_side {
  const orbx_keypoint* d_kps_l;   /* [nframes][cap_l]; x, y, octave and angle are read (mvKeys) */
  const uint8_t* d_desc_l;        /* [nframes][cap_l][32], 16-byte aligned */
  const int32_t* d_counts_l;      /* [nframes][2]: {keypoints, -} */
  const orbx_keypoint* d_kps_r;   /* [nframes][cap_r] (mvKeysRight) */
  const uint8_t* d_desc_r;        /* [nframes][cap_r][32], 16-byte aligned */
  const int32_t* d_counts_r;      /* [nframes][2] */
  const int32_t* d_l2r;           /* [nframes][cap_l]: mvLeftToRightMatch, -1 without one; entry 2 does not read it (may be NULL there) */
  const int32_t* d_r2l;           /* [nframes][cap_r]: mvRightToLeftMatch; as d_l2r */
  const float* d_bounds;          /* [nframes][4] = {min_x, min_y, max_x, max_y}: mnMinX, mnMinY, mnMaxX, mnMaxY, for both grids */
  int nframes, cap_l, cap_r;
} orbx_rigmatch_side;

/* Entry 1: one map point of an item's local map, 48 bytes.  point: its descriptor's row in d_pdesc. */
typedef struct orbx_rigmatch_local_point {
  float proj_x, proj_y, view_cos;
  int32_t level;
  float proj_xr, proj_yr, view_cos_r;
  int32_t level_r;
  int32_t obs, point, in_view, in_view_r;
} orbx_rigmatch_local_point;

/* Entry 2: an item and one point of the last frame, 16 and 48 bytes. */
typedef struct orbx_rigmatch_last_item {
  int32_t frame, direction;   /* 1: bForward, 2: bBackward, 0: neither */
  float th;
  int32_t reserved;
} orbx_rigmatch_last_item;

typedef struct orbx_rigmatch_last_point {
  float u, v, u_r, v_r;
  float angle;                /* of the last frame's keypoint (raw mvKeys / mvKeysRight) */
  int32_t octave, obs, point;
  int32_t valid, reserved[3];
} orbx_rigmatch_last_point;

/* ORBX_E_INVALID for out = NULL or device < 0, ORBX_E_DEVICE when the device cannot be opened (reason: orbx_rigmatch_last_error(NULL)). */
ORBX_RIGMATCH_EXPORT int orbx_rigmatch_create(orbx_rigmatch** out, int device);
ORBX_RIGMATCH_EXPORT void orbx_rigmatch_destroy(orbx_rigmatch* m);
/* The reason of the handle's last failure; with m = NULL the calling thread's last orbx_rigmatch_create failure. */
ORBX_RIGMATCH_EXPORT const char* orbx_rigmatch_last_error(const orbx_rigmatch* m);

/* Entry 1 for items [0, nitems):
 *   d_frames   [nitems] int32: the frame item b is tracked in; one frame may appear in many items
 *   d_mp       [nitems][mcap] orbx_rigmatch_local_point, 16-byte aligned; d_nmp [nitems] int32: row b holds nmp[b] points
 *   d_pdesc    [npoints][32]: the map points' descriptors, 16-byte aligned
 *   scale_factors [nlevels] float32 in HOST memory (mvScaleFactors), read during the call
 *   th, nn_ratio  the call's th and the matcher's mfNNratio
 *   d_kp_obs   [nitems][cap_l + cap_r] int32, IN / OUT: Observations() of the map point slot s of item b holds, -1 without one
 *   d_kp_match [nitems][cap_l + cap_r] int32, OUT: the index in row b of the point this call left in slot s, -1 untouched; whole rows are
 *              written, -1 beyond the frame's counts
 *   d_nmatches [nitems] int32, OUT: what the reference returns
 * Asynchronous on `stream`; NULL is the handle's own stream.
 * ORBX_E_INVALID for what the host can check: NULL arguments, sizes < 1, cap_l + cap_r above 32 768, nlevels outside 1 .. 16, a th that is
 * not finite, a misaligned d_desc_l, d_desc_r, d_mp or d_pdesc, mcap * (cap_l + cap_r) or nitems * max(mcap, cap_l + cap_r) beyond INT_MAX,
 * buffers on another device than the handle's. */
ORBX_RIGMATCH_EXPORT int orbx_rigmatch_local_device(orbx_rigmatch* m, const orbx_rigmatch_side* side, const int32_t* d_frames, int nitems,
                                                    const orbx_rigmatch_local_point* d_mp, const int32_t* d_nmp, int mcap,
                                                    const uint8_t* d_pdesc, int npoints, const float* scale_factors, int nlevels, float th,
                                                    float nn_ratio, int32_t* d_kp_obs, int32_t* d_kp_match, int32_t* d_nmatches, void* stream);

/* The same on host arrays of the same layout (the d_ members of side, the items, descriptors and results are host pointers here): uploads
 * them, searches, and returns when the results are in the caller's buffers; kp_obs is read and updated. */
ORBX_RIGMATCH_EXPORT int orbx_rigmatch_local(orbx_rigmatch* m, const orbx_rigmatch_side* side, const int32_t* frames, int nitems,
                                             const orbx_rigmatch_local_point* mp, const int32_t* nmp, int mcap, const uint8_t* pdesc,
                                             int npoints, const float* scale_factors, int nlevels, float th, float nn_ratio, int32_t* kp_obs,
                                             int32_t* kp_match, int32_t* nmatches);

/* Entry 2 for items [0, nitems): d_items [nitems]; d_points [nitems][mcap], 16-byte aligned; d_nlast [nitems]: row b holds nlast[b]
 * points; check_orientation: the matcher's mbCheckOrientation; the rest as entry 1. */
ORBX_RIGMATCH_EXPORT int orbx_rigmatch_last_device(orbx_rigmatch* m, const orbx_rigmatch_side* side, const orbx_rigmatch_last_item* d_items,
                                                   int nitems, const orbx_rigmatch_last_point* d_points, const int32_t* d_nlast, int mcap,
                                                   const uint8_t* d_pdesc, int npoints, const float* scale_factors, int nlevels,
                                                   int check_orientation, int32_t* d_kp_obs, int32_t* d_kp_match, int32_t* d_nmatches,
                                                   void* stream);

ORBX_RIGMATCH_EXPORT int orbx_rigmatch_last(orbx_rigmatch* m, const orbx_rigmatch_side* side, const orbx_rigmatch_last_item* items, int nitems,
                                            const orbx_rigmatch_last_point* points, const int32_t* nlast, int mcap, const uint8_t* pdesc,
                                            int npoints, const float* scale_factors, int nlevels, int check_orientation, int32_t* kp_obs,
                                            int32_t* kp_match, int32_t* nmatches);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_RIGMATCH_H */
