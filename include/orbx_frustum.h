/* orbx_frustum.h — the batched Frame::isInFrustum (src/Frame.cc:512-574, the Nleft == -1 branch, pinhole camera) together with
 * MapPoint::PredictScale(dist, Frame*) (src/MapPoint.cc:531-546), for B (pose, local map) items at once over a table of map points that
 * stays in HBM.  The output is the orbx_localmatch_point rows orbx_localmatch_search_device reads (include/orbx_localmatch.h), so a batch of
 * poses becomes a batch of matches without the records leaving the device.  Not part of the drop-in boundary (include/orbx.h): these entry
 * points live in liborbx_frustum.so.  The library reads plain device arrays only; it takes nothing from a context or from the product.
 *
 * Out of scope: the two-camera branch (isInFrustumChecks), KannalaBrandt8::project (libm's atan2f bit for bit), ProjectPointDistort, and the
 * Sophus Tcw * x projections of the LastFrame, relocalization, Sim3 and Fuse callers (their rotation arithmetic is another specification).
 *
 * The specification.  For item b, slot j < nmp[b], idx = d_idx[b][j], P the point's record, R / t / Ow the item's: every operation is
 * float32 and rounded once, nothing is contracted, divisions and square roots are correctly rounded.
 *    1. skipped slot: idx < 0 (the caller's mnLastFrameSeen test) or d_obs[idx] < 0 (isBad()): in_view 0, proj_x = proj_y = -1, the other
 *       fields 0.  point = idx in every record of a slot below nmp.
 *    2. Pc[k] = sum3(R[k][0]*P[0], R[k][1]*P[1], R[k][2]*P[2]) + t[k]
 *    3. Pc_dist = sqrt(sum3(Pc[0]^2, Pc[1]^2, Pc[2]^2))
 *    4. invz = 1.0f / Pc[2]; Pc[2] < 0.0f returns false (-0.0f is not below zero and goes on, as in the reference)
 *    5. u = (fx * Pc[0]) / Pc[2] + cx, v = (fy * Pc[1]) / Pc[2] + cy: Pinhole::project divides by z, it does not multiply by invz
 *    6. u < minX || u > maxX returns false, then the same for v; the edges are inclusive.  From here on proj_x = u and proj_y = v even on a
 *       later rejection, as the reference leaves mTrackProjX / mTrackProjY
 *    7. PO = P - Ow, dist = sqrt(sum3(PO^2)); dist < min_inv || dist > max_inv returns false
 *    8. viewCos = sum3(PO[k]*n[k]) / dist; viewCos < cos_limit returns false.  A NaN passes every one of these comparisons, as it does in
 *       the reference
 *    9. level = PredictScale: ratio = max_dist / dist, then clamp(ceil(log(ratio) / log_scale_factor), 0, nlevels - 1)
 *   10. accepted: proj_xr = u - mbf * invz (a product and a subtraction), view_cos = viewCos, obs = d_obs[idx], depth = Pc_dist, in_view = 1,
 *       and the slot counts in ntomatch.  When far_th > 0 && Pc_dist > far_th, in_view becomes 0 and the other fields stay (the bFarPoints
 *       test of Tracking::SearchLocalPoints, which orbx_localmatch.h asks the caller to fold into the flag); the slot still counts.
 *   11. rejected: in_view 0, proj_x / proj_y as step 1 or step 6 left them, every other field and the depth 0.
 * A slot at or beyond nmp[b], and every slot of a malformed item, is 32 zero bytes with depth 0.  Whole records compare bit for bit.
 *
 * sum_order.  sum3(a, b, c) is (a + b) + c under ORBX_FRUSTUM_SUM_LTR and a + (b + c) under ORBX_FRUSTUM_SUM_TREE.  The first is what this
 * project's Eigen stand-ins compute (tests/support/ref_world/Eigen/Core), the arithmetic behind every recorded reference result here; the
 * second is the order in which Eigen's unrolled reduction adds three terms.  Which of the two a given Eigen build uses has not been settled:
 * the project is built and tested without Eigen.  LTR is the default (0).
 *
 * log_kind.  The reference's unqualified log(ratio) on a float is ::log(double) or std::log(float), depending on what the translation unit's
 * includes pull into the global namespace.  ORBX_FRUSTUM_LOG_DOUBLE (the default, 0): log((double)ratio) / (double)log_scale_factor, a
 * double division.  ORBX_FRUSTUM_LOG_FLOAT: logf(ratio) / log_scale_factor, a float division; ceil takes the promoted value.  The two differ on
 * real inputs: at scale factor 1.2 the boundary between levels 1 and 2 is ratio 0x1.333332p+0 under DOUBLE and 0x1.333334p+0 under FLOAT.
 *
 * log on the device.  The level is a step function of ratio.  Per (log_scale_factor, nlevels, log_kind), cached in the handle, the host
 * finds for each n in 0 .. nlevels-2 the largest positive float T[n] with level(ratio) <= n, by bisection over float bit patterns through the
 * host's own libm and the literal expression; the device level is the number of n with ratio > T[n].  That is exact for whatever libm the
 * host has, provided the expression is monotone in ratio: the bisection verifies the step on the 4096 floats on either side of every
 * threshold, and the call fails with ORBX_E_INVALID and a plain reason where the step is not clean.  orbx_frustum_level_thresholds is that
 * routine (host only).  orbx_frustum_project_reference never uses thresholds: it calls libm's log for every point.
 *
 * Limits.  Where ratio is NaN, infinite or <= 0 (dist = 0, a NaN position), or where the quotient leaves the range of int, the reference's
 * float-to-int conversion is undefined; here the level is 0, which is x86's answer (the conversion gives INT_MIN, which the clamp raises to
 * 0).  nlevels is 1 .. 16.  nitems * mcap and the number of workgroups stay within INT_MAX.
 *
 * A handle holds one stream and one event of its own; calls on one handle run one after the other on the device.  The result does not
 * depend on scheduling: ntomatch is an integer count. */
#ifndef ORBX_FRUSTUM_H
#define ORBX_FRUSTUM_H

#include <stddef.h>
#include <stdint.h>

#include "orbx.h"
#include "orbx_localmatch.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#define ORBX_FRUSTUM_EXPORT __attribute__((visibility("default")))
#else
#define ORBX_FRUSTUM_EXPORT
#endif

#define ORBX_FRUSTUM_MAX_LEVELS 16
#define ORBX_FRUSTUM_SUM_LTR 0
#define ORBX_FRUSTUM_SUM_TREE 1
#define ORBX_FRUSTUM_LOG_DOUBLE 0
#define ORBX_FRUSTUM_LOG_FLOAT 1

typedef struct orbx_frustum orbx_frustum;

/* One map point of the resident table: 48 bytes, 16-byte aligned. */
typedef struct orbx_frustum_point {
  float pos[3];      /* mWorldPos */
  float min_inv;     /* GetMinDistanceInvariance() = 0.8f * mfMinDistance, computed by the caller */
  float normal[3];   /* mNormalVector */
  float max_inv;     /* GetMaxDistanceInvariance() = 1.2f * mfMaxDistance */
  float max_dist;    /* the raw mfMaxDistance PredictScale divides */
  float pad[3];
} orbx_frustum_point;

/* One item: a frame's pose and calibration, 112 bytes.  The library never inverts a pose: Ow is the caller's mOw. */
typedef struct orbx_frustum_item {
  float Rcw[9];      /* row-major */
  float tcw[3];
  float Ow[3];
  float fx, fy, cx, cy, mbf;
  float bounds[4];   /* {mnMinX, mnMinY, mnMaxX, mnMaxY} */
  float far_th;      /* <= 0: no far-point test */
  float pad[3];
} orbx_frustum_item;

/* ORBX_E_INVALID for out = NULL or device < 0, ORBX_E_DEVICE when the device cannot be opened (reason: orbx_frustum_last_error(NULL)). */
ORBX_FRUSTUM_EXPORT int orbx_frustum_create(orbx_frustum** out, int device);
ORBX_FRUSTUM_EXPORT void orbx_frustum_destroy(orbx_frustum* f);
/* The reason of the handle's last failure; with f = NULL the calling thread's last failure of a call without a handle. */
ORBX_FRUSTUM_EXPORT const char* orbx_frustum_last_error(const orbx_frustum* f);

/* thresholds[n], n in 0 .. nlevels-2: the largest positive finite float whose level is <= n (FLT_MAX where no finite ratio reaches level
 * n + 1).  Host only, no device needed.  ORBX_E_INVALID (reason: orbx_frustum_last_error(NULL)) for a NULL array with nlevels > 1, nlevels
 * outside 1 .. 16, an unknown log_kind, a log_scale_factor that is not finite and positive, or a step that is not clean. */
ORBX_FRUSTUM_EXPORT int orbx_frustum_level_thresholds(float log_scale_factor, int nlevels, int log_kind, float* thresholds);

/* The projection for items [0, nitems):
 *   d_points  [npoints] orbx_frustum_point, 16-byte aligned; d_obs [npoints] int32: Observations(), negative = isBad()
 *   d_items   [nitems] orbx_frustum_item
 *   d_idx     [nitems][mcap] int32: item b's local map as indices into the table, negative = a slot to skip; d_nmp [nitems] int32
 *   log_scale_factor  the float mfLogScaleFactor as the caller holds it; nlevels 1 .. 16; cos_limit: Tracking passes 0.5f
 *   d_mp      [nitems][mcap] orbx_localmatch_point, 16-byte aligned, OUT: whole rows are written
 *   d_depth   [nitems][mcap] float, OUT, or NULL: mTrackDepth
 *   d_ntomatch [nitems] int32, OUT: the number of `true` returns (Tracking's nToMatch)
 * d_ntomatch[b] = -1 with a row of zero records for a malformed item: nmp outside 0 .. mcap, an index >= npoints among the row's first nmp,
 * or (every item) a log_scale_factor that is not finite and positive.  All of it is checked on the device before any of these values
 * addresses memory.  Asynchronous on `stream`; NULL is the handle's own stream.
 * ORBX_E_INVALID for what the host can check: NULL arguments, sizes < 1, nlevels outside 1 .. 16, an unknown sum_order or log_kind, a NaN
 * cos_limit, a misaligned d_points or d_mp, nitems * mcap beyond INT_MAX, buffers on another device than the handle's, thresholds whose step
 * is not clean. */
ORBX_FRUSTUM_EXPORT int orbx_frustum_project_device(orbx_frustum* f, const orbx_frustum_point* d_points, const int32_t* d_obs, int npoints,
                                                    const orbx_frustum_item* d_items, int nitems, const int32_t* d_idx, const int32_t* d_nmp,
                                                    int mcap, float log_scale_factor, int nlevels, float cos_limit, int sum_order, int log_kind,
                                                    orbx_localmatch_point* d_mp, float* d_depth, int32_t* d_ntomatch, void* stream);

/* The same on host arrays of the same layout: uploads them, projects, and returns when the results are in the caller's buffers. */
ORBX_FRUSTUM_EXPORT int orbx_frustum_project(orbx_frustum* f, const orbx_frustum_point* points, const int32_t* obs, int npoints,
                                             const orbx_frustum_item* items, int nitems, const int32_t* idx, const int32_t* nmp, int mcap,
                                             float log_scale_factor, int nlevels, float cos_limit, int sum_order, int log_kind,
                                             orbx_localmatch_point* mp, float* depth, int32_t* ntomatch);

/* The host twin: the per-frame loop in plain C++ on host arrays, libm's log called for every accepted point, no thresholds and no device.
 * The same results as orbx_frustum_project, malformed items included.  Reason of a failure: orbx_frustum_last_error(NULL). */
ORBX_FRUSTUM_EXPORT int orbx_frustum_project_reference(const orbx_frustum_point* points, const int32_t* obs, int npoints,
                                                       const orbx_frustum_item* items, int nitems, const int32_t* idx, const int32_t* nmp,
                                                       int mcap, float log_scale_factor, int nlevels, float cos_limit, int sum_order,
                                                       int log_kind, orbx_localmatch_point* mp, float* depth, int32_t* ntomatch);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_FRUSTUM_H */
