/* orbx_project.h — the Sophus `Tcw * x` projection fronts of three ORBmatcher callers, for B (pose, point list) items at once over the table
 * of map points liborbx_frustum.so reads (include/orbx_frustum.h: orbx_frustum_point[npoints] and d_obs[npoints], unchanged, so one resident
 * table serves all four projections):
 *    last    SearchByProjection(CurrentFrame, LastFrame, th, bMono), src/ORBmatcher.cc:1703-1721  ->  orbx_lastmatch_point rows
 *    reloc   SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist), :1913-1937         ->  orbx_projmatch_point rows (kind 0)
 *    fuse    Fuse(pKF, vpMapPoints, th, bRight = false), :1198-1244                                ->  orbx_fuse_query rows
 * The rows are what orbx_lastmatch_search_device, orbx_projmatch_search_device and orbx_fuse_search_device read, so a batch of poses becomes
 * a batch of matches without the records leaving the device.  Not part of the drop-in boundary (include/orbx.h): these entry points live in
 * liborbx_project.so.  The library reads plain device arrays only; it takes nothing from a context, from the product or from the matchers.
 *
 * Out of scope: the Sim3 callers (:427, :534, the Sim3 Fuse :1340, SearchBySim3), bRight and two-camera rigs, KannalaBrandt8::project,
 * bForward / bBackward (tlc and the direction of an orbx_lastmatch_item stay the caller's), the side effects of the three routines
 * (the matcher's results are applied by the caller), and a real Eigen: the project is built and tested without Eigen and without Sophus.
 *
 * A slot.  Last and reloc take rows of orbx_project_slot (the point's index in the table, the last frame's / keyframe's keypoint octave and
 * angle); fuse takes rows of int32 indices, as orbx_frustum_project_device's d_idx.  point < 0 marks a slot the caller skipped: the caller
 * folds "no map point", mvbOutlier, isBad(), sAlreadyFound and IsInKeyFrame into that sign.  d_obs is read for the obs field of a last row
 * only; it gates nothing here.
 *
 * The shared arithmetic.  Every operation is float32 and rounded once, nothing is contracted, divisions and square roots are correctly
 * rounded.  sum3(a, b, c) follows sum_order as in orbx_frustum.h: (a + b) + c under ORBX_FRUSTUM_SUM_LTR (the default), a + (b + c) under
 * ORBX_FRUSTUM_SUM_TREE.  P is the point's pos, R / t / Ow / q the item's.
 *    Pc = Tcw * P under rot_kind:
 *      ORBX_PROJECT_ROT_MATRIX (0, the default)  Pc[k] = sum3(R[k][0]*P[0], R[k][1]*P[1], R[k][2]*P[2]) + t[k].  This is what this project's
 *        Sophus stand-ins compute (tests/support/ref_world/sophus/se3.hpp), the arithmetic behind every recorded reference result here.
 *      ORBX_PROJECT_ROT_QUAT (1)  the text of Sophus's SO3::operator* (sophus/so3.hpp: uv = q.vec().cross(p); uv += uv;
 *        return p + q.w()*uv + q.vec().cross(uv)) and SE3's "+ translation", with qv = q[0..2], w = q[3]:
 *          c  = cross(qv, P), in Eigen's component order (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0): two products and a difference
 *          uv = c + c
 *          Pc[k] = ((P[k] + w*uv[k]) + cross(qv, uv)[k]) + t[k]
 *        sum_order does not enter this form.  R is not read under QUAT, q is not read under MATRIX.
 *      Which of the two a given Sophus and Eigen build evaluates, and in which order it adds, has not been settled: neither form has been
 *      checked against a real Eigen build.
 *    u = (fx * Pc[0]) / Pc[2] + cx, v = (fy * Pc[1]) / Pc[2] + cy: Pinhole::project divides by z, it does not multiply by invz.
 *    PO = P - Ow, dist = sqrt(sum3(PO[0]^2, PO[1]^2, PO[2]^2)), dot = sum3(PO[0]*n[0], PO[1]*n[1], PO[2]*n[2]).
 *    level = MapPoint::PredictScale: ratio = max_dist / dist, then clamp(ceil(log(ratio) / log_scale_factor), 0, nlevels - 1), exactly step 9
 *      of orbx_frustum.h with its log_kind and its Limits (a ratio that is NaN, infinite or <= 0 has level 0).  On the device the level is
 *      the number of n with ratio > thresholds[n]; thresholds is a host array of nlevels - 1 floats, exactly what
 *      orbx_frustum_level_thresholds returns for (log_scale_factor, nlevels, log_kind).  This library does not bisect: it rejects thresholds
 *      that are not finite, positive and strictly increasing.  The host twins take log_scale_factor and log_kind instead and call libm's log
 *      for every point.
 *
 * The three emitters, for item b and slot j < nslots[b] with point >= 0 (every `skip` leaves the skipped row):
 *    last   invz = 1.0f / Pc[2] (the reference's 1.0 / x in double, narrowed to float, equals the float quotient: a double holds more than
 *           twice a float's digits); invz < 0 skips, so -0.0f in Pc[2] (invz = -inf) skips and +0.0f goes on to a non-finite u;
 *           u < minX || u > maxX skips, then the same for v: the edges are inclusive and a NaN passes.
 *           row = {u, v, invz, slot.angle, slot.octave, d_obs[point], point, 1}; the skipped row is 32 zero bytes.  No level, no thresholds.
 *    reloc  there is no depth test, as the reference has none: a point behind the camera whose quotient lands in bounds is valid.
 *           The bounds as for last; dist < min_inv || dist > max_inv skips.
 *           row = {u, v, slot.angle, level, point, 1, {0, 0}}; the skipped row is 32 zero bytes.
 *    fuse   Pc[2] < 0.0f skips (-0.0f is not below zero and goes on); invz = 1.0f / Pc[2]; KeyFrame::IsInImage is half-open:
 *           !(u >= minX && u < maxX) skips, then the same for v, so a NaN fails; ur = u - mbf * invz (a product, then a subtraction);
 *           the distance gate as for reloc; (double)dot < 0.5 * (double)dist skips; r = th * scale_factors[level] in float32, scale_factors
 *           a host array of nlevels floats.
 *           query = {u, v, r, ur, level - 1, level, point, 0}; the skipped query has point = -1 and its other fields 0.
 * A slot at or beyond nslots[b] is a skipped row.  Whole rows are written and compare bit for bit.
 *
 * d_nvalid[b] is the number of valid rows of item b (valid = 1; for fuse, point >= 0).  A malformed item has d_nvalid[b] = -1 and a row of
 * skipped records: nslots[b] outside 0 .. mcap, or a point index >= npoints among the row's first nslots[b].  All of it is checked on the
 * device before any of these values addresses memory.  nlevels is 1 .. 16.  nitems * mcap and the number of workgroups stay within INT_MAX.
 *
 * A handle holds one stream and one event of its own; calls on one handle run one after the other on the device.  The result does not
 * depend on scheduling: d_nvalid is an integer count. */
#ifndef ORBX_PROJECT_H
#define ORBX_PROJECT_H

#include <stddef.h>
#include <stdint.h>

#include "orbx.h"
#include "orbx_frustum.h"
#include "orbx_fuse.h"
#include "orbx_lastmatch.h"
#include "orbx_projmatch.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#define ORBX_PROJECT_EXPORT __attribute__((visibility("default")))
#else
#define ORBX_PROJECT_EXPORT
#endif

#define ORBX_PROJECT_ROT_MATRIX 0
#define ORBX_PROJECT_ROT_QUAT 1

typedef struct orbx_project orbx_project;

/* One item: a pose in both its forms, the calibration and the image bounds, 128 bytes.  The library never inverts a pose: Ow is the
 * caller's camera centre. */
typedef struct orbx_project_item {
  float Rcw[9];      /* row-major */
  float tcw[3];
  float Ow[3];
  float q[4];        /* x, y, z, w of Tcw.unit_quaternion() */
  float fx, fy, cx, cy, mbf;
  float bounds[4];   /* {mnMinX, mnMinY, mnMaxX, mnMaxY} */
  float th;          /* fuse: the radius factor; not read by last and reloc (their th is the matcher item's) */
  float pad[3];
} orbx_project_item;

/* One slot of a last or reloc row, 16 bytes, 16-byte aligned. */
typedef struct orbx_project_slot {
  int32_t point;     /* index into the table; negative = a slot to skip */
  int32_t octave;    /* last: LastFrame.mvKeys[i].octave */
  float angle;       /* the keypoint's angle, copied into the row */
  int32_t pad;
} orbx_project_slot;

/* ORBX_E_INVALID for out = NULL or device < 0, ORBX_E_DEVICE when the device cannot be opened (reason: orbx_project_last_error(NULL)). */
ORBX_PROJECT_EXPORT int orbx_project_create(orbx_project** out, int device);
ORBX_PROJECT_EXPORT void orbx_project_destroy(orbx_project* p);
/* The reason of the handle's last failure; with p = NULL the calling thread's last failure of a call without a handle. */
ORBX_PROJECT_EXPORT const char* orbx_project_last_error(const orbx_project* p);

/* The arguments all forms share:
 *   d_points  [npoints] orbx_frustum_point, 16-byte aligned; d_obs [npoints] int32 (last only)
 *   d_items   [nitems] orbx_project_item
 *   d_slots   [nitems][mcap] orbx_project_slot, 16-byte aligned (fuse: d_idx [nitems][mcap] int32); d_nslots [nitems] int32
 *   d_out     [nitems][mcap] rows of the consumer, 16-byte aligned, OUT; d_nvalid [nitems] int32, OUT
 * The _device forms are asynchronous on `stream`; NULL is the handle's own stream.  ORBX_E_INVALID for what the host can check: NULL
 * arguments, sizes < 1, nlevels outside 1 .. 16, an unknown rot_kind, sum_order or log_kind, misaligned d_points, d_slots or d_out,
 * nitems * mcap beyond INT_MAX, buffers on another device than the handle's, thresholds that are not finite, positive and strictly
 * increasing.  The forms without _device take host arrays of the same layout: they upload them, project, and return when the results are in
 * the caller's buffers.  The _reference forms are the host twins: the per-point loop in plain C++ on host arrays, libm's log called for
 * every point that reaches the level, no thresholds and no device; the same results, malformed items included, and ORBX_E_INVALID for a
 * log_scale_factor that is not finite and positive.  Reason of a twin's failure: orbx_project_last_error(NULL). */
ORBX_PROJECT_EXPORT int orbx_project_last_device(orbx_project* p, const orbx_frustum_point* d_points, const int32_t* d_obs, int npoints,
                                                 const orbx_project_item* d_items, int nitems, const orbx_project_slot* d_slots,
                                                 const int32_t* d_nslots, int mcap, int rot_kind, int sum_order, orbx_lastmatch_point* d_out,
                                                 int32_t* d_nvalid, void* stream);
ORBX_PROJECT_EXPORT int orbx_project_last(orbx_project* p, const orbx_frustum_point* points, const int32_t* obs, int npoints,
                                          const orbx_project_item* items, int nitems, const orbx_project_slot* slots, const int32_t* nslots,
                                          int mcap, int rot_kind, int sum_order, orbx_lastmatch_point* out, int32_t* nvalid);
ORBX_PROJECT_EXPORT int orbx_project_last_reference(const orbx_frustum_point* points, const int32_t* obs, int npoints,
                                                    const orbx_project_item* items, int nitems, const orbx_project_slot* slots,
                                                    const int32_t* nslots, int mcap, int rot_kind, int sum_order, orbx_lastmatch_point* out,
                                                    int32_t* nvalid);

ORBX_PROJECT_EXPORT int orbx_project_reloc_device(orbx_project* p, const orbx_frustum_point* d_points, int npoints,
                                                  const orbx_project_item* d_items, int nitems, const orbx_project_slot* d_slots,
                                                  const int32_t* d_nslots, int mcap, const float* thresholds, int nlevels, int rot_kind,
                                                  int sum_order, orbx_projmatch_point* d_out, int32_t* d_nvalid, void* stream);
ORBX_PROJECT_EXPORT int orbx_project_reloc(orbx_project* p, const orbx_frustum_point* points, int npoints, const orbx_project_item* items,
                                           int nitems, const orbx_project_slot* slots, const int32_t* nslots, int mcap, const float* thresholds,
                                           int nlevels, int rot_kind, int sum_order, orbx_projmatch_point* out, int32_t* nvalid);
ORBX_PROJECT_EXPORT int orbx_project_reloc_reference(const orbx_frustum_point* points, int npoints, const orbx_project_item* items, int nitems,
                                                     const orbx_project_slot* slots, const int32_t* nslots, int mcap, float log_scale_factor,
                                                     int nlevels, int log_kind, int rot_kind, int sum_order, orbx_projmatch_point* out,
                                                     int32_t* nvalid);

ORBX_PROJECT_EXPORT int orbx_project_fuse_device(orbx_project* p, const orbx_frustum_point* d_points, int npoints,
                                                 const orbx_project_item* d_items, int nitems, const int32_t* d_idx, const int32_t* d_nslots,
                                                 int mcap, const float* thresholds, const float* scale_factors, int nlevels, int rot_kind,
                                                 int sum_order, orbx_fuse_query* d_out, int32_t* d_nvalid, void* stream);
ORBX_PROJECT_EXPORT int orbx_project_fuse(orbx_project* p, const orbx_frustum_point* points, int npoints, const orbx_project_item* items,
                                          int nitems, const int32_t* idx, const int32_t* nslots, int mcap, const float* thresholds,
                                          const float* scale_factors, int nlevels, int rot_kind, int sum_order, orbx_fuse_query* out,
                                          int32_t* nvalid);
ORBX_PROJECT_EXPORT int orbx_project_fuse_reference(const orbx_frustum_point* points, int npoints, const orbx_project_item* items, int nitems,
                                                    const int32_t* idx, const int32_t* nslots, int mcap, float log_scale_factor,
                                                    const float* scale_factors, int nlevels, int log_kind, int rot_kind, int sum_order,
                                                    orbx_fuse_query* out, int32_t* nvalid);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_PROJECT_H */
