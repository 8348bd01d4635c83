/* orbx_mpgeom.h — the batched MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:426-494) for M map points at once, written in place into the
 * resident table of map points (orbx_frustum_point, include/orbx_frustum.h) that FrustumBatch, ProjectBatch and Sim3Batch read: the view
 * direction `normal` and the scale-invariance range (min_inv, max_inv, max_dist) that isInFrustum and PredictScale decide on.  The reference
 * calls it wherever it calls ComputeDistinctiveDescriptors (src/LocalMapping.cc:322,706,816, src/LoopClosing.cc:1099,1703,
 * src/Tracking.cc:2394,2415,2563,3317) and for every point a bundle adjustment moved (src/Optimizer.cc:382,800,1494,1778,2105,2954,3942,
 * 4485,5585, src/Map.cc:280).  Not part of the drop-in boundary (include/orbx.h): these entry points live in liborbx_mpgeom.so.  The library
 * reads plain device arrays only; it takes nothing from a context or from the product.
 *
 * Out of scope:
 *   mObservations, mpRefKF, isBad(), the mutexes and Observations(): host pointer work, and the reference's nObs depends on the history of
 *     additions.  The caller lists the observations and names the reference keyframe;
 *   SetWorldPos: the caller writes `pos`;
 *   GetCameraCenter's own computation: the caller's pose arithmetic.  The centres come in as they are.
 *
 * The side.  d_kps [nframes][capacity] and d_counts [nframes][2] are the buffers a batch extraction or orbx_rigbow_stack_device leaves; of a
 * keypoint only `octave` is read.  d_nleft [nframes] is Nleft of each frame, -1 for a single-camera frame, NULL when every frame is
 * single-camera (orbx_rigbow_side's convention).  d_centres [nframes][8] float, 16-byte aligned:
 * {GetCameraCenter().xyz, 0, GetRightCameraCenter().xyz, 0}; the right half is read only for a rig frame's right rows.
 *
 * The observations.  d_obs [nobs] {frame, row} (orbx_mpdesc_obs's 8 bytes), d_obs_start [npoints + 1] the CSR ranges, in the order of the
 * reference's loop (:447-466): its std::map order, a keyframe's left row before its right row.  A right observation is row rightIndex of the
 * stacked frame, Nleft + j.  The same (frame, row) may appear in many points and twice in one.  This list does NOT leave out bad keyframes:
 * UpdateNormalAndDepth walks every observation, ComputeDistinctiveDescriptors skips the bad ones (orbx_mpdesc.h), so one CSR serves both
 * calls only where no observing keyframe is bad.
 * d_ref [npoints] {frame, row}: mpRefKF and the row the reference takes the level from (:471-482): leftIndex when it is not -1, otherwise
 * the stacked rightIndex.  Where mpRefKF is not among the observations the reference's observations[pRefKF] inserts (0, 0): the caller
 * passes row 0.
 * d_row [npoints] or NULL: the table row of point m (NULL: row m).  The caller keeps the rows of one call distinct.
 *
 * The specification is the reference's loop.  Every operation is float32 and rounded once, nothing is contracted, divisions and square
 * roots are correctly rounded, subnormals are kept.  For point m: N its number of observations, r its table row, P = table[r].pos.
 *   1. N == 0: the reference returns early (:441): d_n[m] = 0, the row and d_min_dist[m] are untouched; d_ref[m] is not looked at.
 *   2. normal = (0, 0, 0).  For each observation in list order: C the left centre of its frame, or the right centre when d_nleft is given,
 *      nleft[frame] >= 0 and row >= nleft[frame]; d = P - C; len = sqrt(sum3(d0*d0, d1*d1, d2*d2)); normal[k] = normal[k] + q(d[k], len).
 *      The additions are strictly sequential in list order.  n = N.
 *   3. PC = P - (the LEFT centre of d_ref[m].frame), also when the reference observation is a right row (:468); dist = sqrt(sum3(PC^2)).
 *   4. level = d_kps[ref.frame][ref.row].octave; max_dist = dist * scale_factors[level]; min_dist = max_dist / scale_factors[nlevels - 1];
 *      normal_out[k] = q(normal[k], (float)n).
 *   5. written to row r: normal = normal_out, max_dist, max_inv = 1.2f * max_dist, min_inv = 0.8f * min_dist; pos and pad keep their bytes.
 *      d_n[m] = n, d_min_dist[m] = min_dist (the raw mfMinDistance, which the table does not hold).
 * A point at a camera centre (len == 0) gives NaNs, as in the reference.
 *
 * sum_order.  sum3 is orbx_frustum.h's: (a + b) + c under ORBX_FRUSTUM_SUM_LTR (0, the default), a + (b + c) under ORBX_FRUSTUM_SUM_TREE.
 * div_kind.  q(a, b) is a / b under ORBX_MPGEOM_DIV_QUOTIENT (0, the default): what this project's Eigen stand-ins
 * (tests/support/ref_world/Eigen/Core) and current Eigen compute for vector / scalar.  Under ORBX_MPGEOM_DIV_RECIPROCAL (1) it is
 * a * (1.0f / b): what the vector-by-scalar quotient of older Eigen releases is recalled to compute.  Which of the two a given Eigen build
 * uses has not been settled: the project is built and tested without Eigen.
 *
 * Malformed points.  d_n[m] = -2, an untouched row and an untouched d_min_dist[m]; every other point of the call is unaffected.  Checked for
 * every point: d_obs_start[m] < 0, d_obs_start[m + 1] < d_obs_start[m], d_obs_start[m + 1] > nobs; N above ORBX_MPGEOM_MAX_OBS; a row
 * outside 0 .. table_rows - 1.  Checked where N > 0: an observation's frame, or the reference frame, outside 0 .. nframes - 1; an
 * observation's row, or the reference row, outside 0 .. min(d_counts[frame][0], capacity) - 1; with d_nleft, an nleft outside
 * [-1, min(d_counts[frame][0], capacity)] on a frame the point names; a reference octave outside [0, nlevels).  All of it is checked on the
 * device before any of these values addresses memory.
 *
 * Limit: at most ORBX_MPGEOM_MAX_OBS = 1024 observations a point, the limit of orbx_mpdesc.h.  nframes * capacity stays within INT_MAX.
 *
 * A handle holds scratch memory, one stream and one event of its own; calls on one handle run one after the other on the device.  No float
 * atomic: the result does not depend on scheduling.  Environment, read at orbx_mpgeom_create (results do not change):
 * ORBX_MPGEOM_SMALL_MAX = the largest N of the lane-per-observation form (0 .. 64, 16 by default); points above it take the wave-per-point
 * form.  The value is read with atoi and clamped: text that is no number counts as 0, which sends every point to the wave-per-point form. */
#ifndef ORBX_MPGEOM_H
#define ORBX_MPGEOM_H

#include <stddef.h>
#include <stdint.h>

#include "orbx.h"
#include "orbx_frustum.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#define ORBX_MPGEOM_EXPORT __attribute__((visibility("default")))
#else
#define ORBX_MPGEOM_EXPORT
#endif

#define ORBX_MPGEOM_MAX_OBS 1024
#define ORBX_MPGEOM_MAX_LEVELS 16
#define ORBX_MPGEOM_DIV_QUOTIENT 0
#define ORBX_MPGEOM_DIV_RECIPROCAL 1

typedef struct orbx_mpgeom orbx_mpgeom;

typedef struct orbx_mpgeom_side {
  const orbx_keypoint* d_kps;   /* [nframes][capacity]: only octave is read */
  const int32_t* d_counts;      /* [nframes][2]: {rows, -} */
  const int32_t* d_nleft;       /* [nframes]: Nleft, -1 for a single-camera frame; NULL: every frame is single-camera */
  const float* d_centres;       /* [nframes][8], 16-byte aligned: {left centre xyz, 0, right centre xyz, 0} */
  int nframes, capacity;
} orbx_mpgeom_side;

/* One observation, and a point's reference: row `row` of keyframe `frame`.  The record of orbx_mpdesc_obs. */
typedef struct orbx_mpgeom_obs {
  int32_t frame, row;
} orbx_mpgeom_obs;

/* ORBX_E_INVALID for out = NULL or device < 0, ORBX_E_DEVICE when the device cannot be opened (reason: orbx_mpgeom_last_error(NULL)). */
ORBX_MPGEOM_EXPORT int orbx_mpgeom_create(orbx_mpgeom** out, int device);
ORBX_MPGEOM_EXPORT void orbx_mpgeom_destroy(orbx_mpgeom* g);
/* The reason of the handle's last failure; with g = NULL the calling thread's last failure of a call without a handle. */
ORBX_MPGEOM_EXPORT const char* orbx_mpgeom_last_error(const orbx_mpgeom* g);

/* The update for points [0, npoints):
 *   d_table        [table_rows] orbx_frustum_point, 16-byte aligned, updated in place
 *   scale_factors  [nlevels] HOST floats, nlevels 1 .. 16: they travel as kernel arguments
 *   d_n            [npoints] int32, OUT: n, 0 (no observation) or -2 (malformed)
 *   d_min_dist     [npoints] float, OUT, or NULL
 * Asynchronous on `stream`; NULL is the handle's own stream.  A fixed number of launches whatever the points are, no host synchronisation.
 * ORBX_E_INVALID for what the host can check: NULL arguments, nframes, capacity, nobs, npoints or table_rows < 1, nframes * capacity beyond
 * INT_MAX, nlevels outside 1 .. 16, an unknown sum_order or div_kind, a table or centres that are not 16-byte aligned, buffers on another
 * device than the handle's. */
ORBX_MPGEOM_EXPORT int orbx_mpgeom_update_device(orbx_mpgeom* g, const orbx_mpgeom_side* side, const orbx_mpgeom_obs* d_obs, int nobs,
                                                 const int32_t* d_obs_start, int npoints, const orbx_mpgeom_obs* d_ref, const int32_t* d_row,
                                                 orbx_frustum_point* d_table, int table_rows, const float* scale_factors, int nlevels,
                                                 int sum_order, int div_kind, int32_t* d_n, float* d_min_dist, void* stream);

/* The same on host arrays of the same layout (the d_ members of side too): uploads them -- the table and min_dist as well, so that what
 * no point writes comes back as it was --, updates, and returns when the results are in the caller's buffers. */
ORBX_MPGEOM_EXPORT int orbx_mpgeom_update(orbx_mpgeom* g, const orbx_mpgeom_side* side, const orbx_mpgeom_obs* obs, int nobs,
                                          const int32_t* obs_start, int npoints, const orbx_mpgeom_obs* ref, const int32_t* row,
                                          orbx_frustum_point* table, int table_rows, const float* scale_factors, int nlevels, int sum_order,
                                          int div_kind, int32_t* n, float* min_dist);

/* The host twin: the per-point loop in plain C++ on host arrays, no device.  The same results as orbx_mpgeom_update, malformed points
 * included, after the same argument checks.  Reason of a failure: orbx_mpgeom_last_error(NULL). */
ORBX_MPGEOM_EXPORT int orbx_mpgeom_update_reference(const orbx_mpgeom_side* side, const orbx_mpgeom_obs* obs, int nobs, const int32_t* obs_start,
                                                    int npoints, const orbx_mpgeom_obs* ref, const int32_t* row, orbx_frustum_point* table,
                                                    int table_rows, const float* scale_factors, int nlevels, int sum_order, int div_kind,
                                                    int32_t* n, float* min_dist);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_MPGEOM_H */
