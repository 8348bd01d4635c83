/* orbx_fuse.h — the batched Fuse search: the inner loop of ORBmatcher::Fuse (src/ORBmatcher.cc:1148), of the Sim3 Fuse (:1340) and of
 * SearchBySim3 (:1457) for P (query row, keyframe) pairs at once, on the keypoints and descriptors a batch extraction left in HBM.
 * LocalMapping::SearchInNeighbors (src/LocalMapping.cc) calls Fuse once per neighbour of the new keyframe and once more with every
 * neighbour's points against the new keyframe: that is the batch.  Not part of the drop-in boundary (include/orbx.h): these entry points
 * live in liborbx_fuse.so.  The library reads plain device arrays only; it takes nothing from a context.
 *
 * In scope: what is a pure function of (query, keyframe) -- the window, the level range, the reprojection gate, the Hamming arg-min and a
 * count of hits.
 * Out of scope:
 *   the projection of the map points (Tcw * p3Dw, project, PredictScale, the viewing-angle and distance checks): the caller does it with
 *     its own Eigen and libm, as orbx_window_nearest's callers do, and hands over x, y, r, ur and the level range;
 *   the side effects (Replace, AddObservation, AddMapPoint, vpReplacePoint): host pointer work, applied by the caller in query order from
 *     best_idx / best_dist;
 *   SearchBySim3's mutual-agreement pass;
 *   two-camera rigs (bRight, NLeft != -1);
 *   grids the caller built itself (orbx_grid with cell_start != NULL): the grids are assigned here, on the device.
 *
 * The specification is the reference's loops.  For pair p, query q of row p and keyframe k = pairs[p]:
 *   grid     feature i of keyframe k lies in cell (round((x - min_x) * inv_w), round((y - min_y) * inv_h)) (Frame::PosInGrid,
 *            src/Frame.cc:725-735): float32, every operation rounded, nothing contracted.  A feature outside 64 x 48 (or whose products are
 *            not finite) is in no cell.  Inside a cell the features stand in ascending index.
 *   window   KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:704-748) with its four early returns, floor / ceil of the float products
 *            (x - min_x - r) * inv_w ..., the ix-major, iy-minor cell walk and fabs(distx) < r && fabs(disty) < r with distx = kp.x - x.
 *   level    a candidate is skipped when octave < min_level || octave > max_level (:1269).  NOTE: orbx_window_nearest reads
 *            max_level < 0 as "no upper bound" (Frame::GetFeaturesInArea's convention); here both bounds always hold, so a query with
 *            max_level < 0 has no candidate of a non-negative octave.
 *   gate     with reprojection_gate set (:1272-1296), ex = x - kp.x, ey = y - kp.y, er = ur - uright, all sums and products float32, left
 *            to right, each comparison one of doubles against the double literal:
 *              stereo keypoint (uright >= 0): e2 = ex*ex + ey*ey + er*er, dropped when (double)(e2 * inv_level_sigma2[octave]) > 7.8;
 *              otherwise:                     e2 = ex*ex + ey*ey,         dropped when (double)(e2 * inv_level_sigma2[octave]) > 5.99.
 *   winner   the smallest Hamming distance between d_pdesc[point] and the candidate's descriptor; the first candidate in walk order wins a
 *            tie (strict <, :1304).  Without a candidate the result is -1 / 256.
 * Nothing is ordered: no "taken" state, no chain, no replay; the result does not depend on scheduling.
 *
 * Limits: the reference leaves a query with a non-finite x, y or r undefined; here it has no candidate.  Coordinates whose cell products
 * leave the range of int are undefined in the reference too; here the conversion saturates.  At most 32 768 keypoints a keyframe, as
 * the device grids of the product.
 *
 * A handle holds the grids of one side, scratch memory, one stream and one event of its own; calls on one handle run one after the other on
 * the device.  Environment, read at orbx_fuse_create (results do not change): ORBX_FUSE_LDS = the largest LDS block in bytes a search may
 * stage a keyframe in (0 .. 155648; keyframes that need more are searched in global memory). */
#ifndef ORBX_FUSE_H
#define ORBX_FUSE_H

#include <stddef.h>
#include <stdint.h>

#include "orbx.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#define ORBX_FUSE_EXPORT __attribute__((visibility("default")))
#else
#define ORBX_FUSE_EXPORT
#endif

#define ORBX_FUSE_MAX_LEVELS 16
#define ORBX_FUSE_MAX_CAPACITY 32768

typedef struct orbx_fuse orbx_fuse;

/* The keyframe side: K keyframes at fixed stride, the buffers a batch extraction leaves. */
typedef struct orbx_fuse_side {
  const orbx_keypoint* d_kps;   /* [nframes][capacity]; x, y and octave are read (mvKeysUn) */
  const uint8_t* d_desc;        /* [nframes][capacity][32], 16-byte aligned */
  const int32_t* d_counts;      /* [nframes][2]: {keypoints, -} */
  const float* d_uright;        /* [nframes][capacity], or NULL: monocular (every value negative).  mvuRight: stereo means uright >= 0 */
  const float* d_gridparm;      /* [nframes][4] = {min_x, min_y, inv_w, inv_h}: orbx_grid's members of the same names with cell_start == NULL */
  int nframes, capacity;
} orbx_fuse_side;

/* One projected map point.  point: its descriptor's row in d_pdesc; point < 0: the caller skipped the query (no point, bad, already in the
 * keyframe, failed a projection check).  ur is read under the gate, for stereo keypoints only. */
typedef struct orbx_fuse_query {
  float x, y, r, ur;
  int32_t min_level, max_level, point, pad;
} orbx_fuse_query;

/* ORBX_E_INVALID for out = NULL or device < 0, ORBX_E_DEVICE when the device cannot be opened (reason: orbx_fuse_last_error(NULL)). */
ORBX_FUSE_EXPORT int orbx_fuse_create(orbx_fuse** out, int device);
ORBX_FUSE_EXPORT void orbx_fuse_destroy(orbx_fuse* m);
/* The reason of the handle's last failure; with m = NULL the calling thread's last orbx_fuse_create failure. */
ORBX_FUSE_EXPORT const char* orbx_fuse_last_error(const orbx_fuse* m);

/* Builds the grids of the side's keyframes in the handle's memory: per keyframe the features sorted by (cell, index).  Every later
 * orbx_fuse_search_device on the same side (the same pointers and sizes) uses them, until the next build on this handle.  The side's
 * buffers are read during the call and must not change between a build and the searches that use it.  A keyframe whose count lies outside
 * 0 .. capacity has no grid: every pair that names it is malformed.  Asynchronous on `stream`; NULL is the handle's own stream.
 * ORBX_E_INVALID: NULL arguments, sizes < 1, a capacity above 32 768, buffers on another device than the handle's. */
ORBX_FUSE_EXPORT int orbx_fuse_grids_device(orbx_fuse* m, const orbx_fuse_side* side, void* stream);

/* The search for pairs [0, npairs):
 *   d_query  [npairs][qcap] orbx_fuse_query, d_nquery [npairs] int32: row p holds nquery[p] queries
 *   d_pairs  [npairs] int32: the keyframe row p is searched in; one keyframe may appear in many pairs
 *   d_pdesc  [npoints][32]: the map points' descriptors, 16-byte aligned, stored once for all the keyframes they are projected into
 *   inv_level_sigma2 [nlevels] float32 in HOST memory (mvInvLevelSigma2), read during the call; needed with reprojection_gate only
 *   th_low   the caller passes TH_LOW = 50; used for the count only
 *   d_best_idx, d_best_dist [npairs][qcap] int32: whole rows are written, -1 / 256 past nquery[p] and for skipped queries
 *   d_nfound [npairs] int32: the number of queries with best_dist <= th_low -- what Fuse would return if no keypoint's existing point
 *            were bad
 * d_nfound[p] = -1 with a row of -1 / 256 for a malformed pair: a keyframe index outside the side, a count outside 0 .. capacity (as the
 * grid build saw it), nquery outside 0 .. qcap, a `point` of the row's first nquery queries that is not below npoints, or, with the gate
 * on, a feature in a cell of the keyframe whose octave lies outside [0, nlevels).  All of it is checked on the device before any of these
 * values addresses memory.  Asynchronous on `stream`; NULL is the handle's own stream.
 * ORBX_E_INVALID for what the host can check: no grid build for this side on this handle, NULL arguments, sizes < 1, with the gate
 * nlevels outside 1 .. 16 or no table, npairs * qcap beyond INT_MAX, buffers on another device than the handle's. */
ORBX_FUSE_EXPORT int orbx_fuse_search_device(orbx_fuse* m, const orbx_fuse_side* side, const orbx_fuse_query* d_query, const int32_t* d_nquery,
                                             int qcap, const int32_t* d_pairs, int npairs, const uint8_t* d_pdesc, int npoints,
                                             const float* inv_level_sigma2, int nlevels, int reprojection_gate, int th_low,
                                             int32_t* d_best_idx, int32_t* d_best_dist, int32_t* d_nfound, void* stream);

/* The same on host arrays of the same layout (the d_ members of side, the queries, pairs, descriptors and results are host pointers here):
 * uploads them, builds the grids of the uploaded side, searches, and returns when the results are in the caller's buffers.  The handle's
 * grids are those of the upload afterwards: a device search on another side needs its own orbx_fuse_grids_device. */
ORBX_FUSE_EXPORT int orbx_fuse_search(orbx_fuse* m, const orbx_fuse_side* side, const orbx_fuse_query* query, const int32_t* nquery, int qcap,
                                      const int32_t* pairs, int npairs, const uint8_t* pdesc, int npoints, const float* inv_level_sigma2,
                                      int nlevels, int reprojection_gate, int th_low, int32_t* best_idx, int32_t* best_dist, int32_t* nfound);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_FUSE_H */
