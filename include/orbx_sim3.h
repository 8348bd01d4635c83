/* orbx_sim3.h — the projection fronts of LoopClosing's four ORBmatcher callers and SearchBySim3's agreement pass, for B items at once over
 * the table of map points liborbx_frustum.so and liborbx_project.so read (include/orbx_frustum.h: orbx_frustum_point[npoints], unchanged,
 * so one resident table serves every projection):
 *    proj    SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming), src/ORBmatcher.cc:427-486, and its vpPointsKFs twin,
 *            :534-599 (before the search the two differ in how they project: proj_kind)        ->  orbx_projmatch_point rows (kind 1)
 *    fuse    Fuse(pKF, Scw, vpPoints, th, vpReplacePoint), :1340-1404                           ->  orbx_fuse_query rows, the gate off
 *    search  one direction of SearchBySim3(pKF1, pKF2, vpMatches12, S12, th), :1496-1537 or :1576-1617  ->  orbx_fuse_query rows, the gate off
 *    agree   SearchBySim3's mutual-agreement pass, :1655-1671, on the results of two orbx_fuse_search_device calls
 * The rows are what orbx_projmatch_search_device and orbx_fuse_search_device read, so a loop-closing batch becomes matches without the
 * records leaving the device.  Not part of the drop-in boundary (include/orbx.h): these entry points live in liborbx_sim3.so.  The library
 * reads plain device arrays only; it takes nothing from a context, from the product, from the matchers or from liborbx_project.so.
 *
 * Out of scope: bRight and two-camera rigs, KannalaBrandt8::project, the side effects of the four routines (vpMatched and vpMatchedKF,
 * vpReplacePoint, AddObservation / AddMapPoint, merging match12 into vpMatches12: the caller applies them), Sim3::inverse and the
 * decomposition of Scw (the caller's, with its own Sophus: the library never inverts a pose or a similarity and divides no translation by a
 * scale), fusing a front into the search's launch, and a real Eigen: the project is built and tested without Eigen and without Sophus.
 *
 * A slot is one int32: the point's index in the table, which is also its descriptor's row for the matchers.  A negative index marks a slot
 * the caller skipped: the caller folds NULL, isBad(), spAlreadyFound and vbAlreadyMatched into that sign.  For search, slot j is keypoint j
 * of the source keyframe (mvpMapPoints[j]), so the searches' best_idx rows are indexed by keypoint, as agree needs them.
 *
 * The shared arithmetic is include/orbx_project.h's: every operation is float32 and rounded once, nothing is contracted, divisions and
 * square roots are correctly rounded.  sum3(a, b, c) follows sum_order: (a + b) + c under ORBX_FRUSTUM_SUM_LTR (the default), a + (b + c)
 * under ORBX_FRUSTUM_SUM_TREE.  A rigid pose T = (R, t, q) applied to P under rot_kind:
 *      ORBX_PROJECT_ROT_MATRIX (0, the default)  T*P[k] = sum3(R[k][0]*P[0], R[k][1]*P[1], R[k][2]*P[2]) + t[k]
 *      ORBX_PROJECT_ROT_QUAT (1)  c = cross(qv, P) in Eigen's component order (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0), uv = c + c,
 *        T*P[k] = ((P[k] + w*uv[k]) + cross(qv, uv)[k]) + t[k], with qv = q[0..2], w = q[3]
 * A similarity S = (s, R, t, q) applied to Pa under sim_kind (search alone):
 *      ORBX_SIM3_MATRIX (0, the default)  Pb[k] = (sum3(R[k][0]*Pa[0], R[k][1]*Pa[1], R[k][2]*Pa[2]) * s) + t[k]: the scale is applied after
 *        the rotation, as this project's Sophus stand-in writes it (tests/support/ref_world/sophus/sim3.hpp: (R_ * p) * s_ + t_), the
 *        arithmetic behind every recorded reference result here.
 *      ORBX_SIM3_QUAT (1)  the text of Sophus's RxSO3::operator* (sophus/rxso3.hpp) and Sim3's "+ translation()", with the item's s where
 *        RxSO3 takes quaternion().squaredNorm(): uv = cross(qv, Pa), uv = uv + uv,
 *        Pb[k] = (s*Pa[k] + (w*uv[k] + cross(qv, uv)[k])) + t[k].  The grouping differs from SO3's form above.  q is the NON-unit
 *        quaternion of the RxSO3 (norm sqrt(s)); sum_order does not enter this form; R is not read under QUAT, q is not read under MATRIX.
 *      Which form a given Sophus and Eigen build evaluates, and in which order it adds, has not been settled: neither form of either
 *      option has been checked against a real Eigen build.
 *    level = MapPoint::PredictScale(dist, pKF): ratio = max_dist / dist, then step 9 of orbx_frustum.h with its log_kind and its Limits.  On
 *      the device the level is the number of n with ratio > thresholds[n]; thresholds is a host array of nlevels - 1 floats, exactly what
 *      orbx_frustum_level_thresholds returns for (log_scale_factor, nlevels, log_kind).  This library does not bisect: it rejects thresholds
 *      that are not finite, positive and strictly increasing.  The host twins take log_scale_factor and log_kind and call libm's log.
 *
 * The three emitters, for item b and slot j < nslots[b] with a non-negative index (every `skip` leaves the skipped row):
 *    proj    the item is an orbx_project_item: the caller supplies Tcw = SE3(Scw.rotationMatrix(), Scw.translation() / Scw.scale()) and Ow.
 *            Pc = Tcw * P; (double)Pc[2] < 0.0 skips (:461 compares against a double zero: -0.0f goes on, a NaN goes on);
 *            under proj_kind:
 *              ORBX_SIM3_PROJ_DIVIDE (0, the default)  :427's pKF->mpCamera->project(p3Dc) (:465): u = (fx * Pc[0]) / Pc[2] + cx, v likewise:
 *                Pinhole::project divides by z;
 *              ORBX_SIM3_PROJ_INVZ (1)  :534's own text (:573-578): invz = 1.0f / Pc[2] (`1 / p3Dc(2)`, a float division), x = Pc[0] * invz,
 *                y = Pc[1] * invz, u = fx * x + cx, v = fy * y + cy: a product and then a sum, never an FMA, as search below;
 *              the two differ in the last bits of u and v, and a point on a bound can change sides; everything else is one text;
 *            KeyFrame::IsInImage is half-open: !(u >= minX && u < maxX) skips, then the same for v, so a NaN fails;
 *            PO = P - Ow, dist = sqrt(sum3(PO[k]^2)); dist < min_inv || dist > max_inv skips;
 *            dot = sum3(PO[k]*normal[k]); (double)dot < 0.5 * (double)dist skips;
 *            row = {u, v, 0.0f, level, point, 1, {0, 0}}; the skipped row is 32 zero bytes.  mbf and th of the item are not read: the
 *            radius stays the matcher's, th * scale_factors[level] from its own item.
 *    fuse    the gates are proj's under ORBX_SIM3_PROJ_DIVIDE (:1379 calls Pinhole::project), the depth test as :1375 writes it
 *            (Pc[2] < 0.0f); r = th * scale_factors[level] in float32, th the item's float;
 *            query = {u, v, r, 0.0f, level - 1, level, point, 0}; the skipped query has point = -1 and its other fields 0.
 *            There is no ur and no mbf: orbx_fuse_search_device is called with reprojection_gate = 0.
 *    search  the item is an orbx_sim3_item; one item is one direction, a SearchBySim3 call is two items (T_1w with S21 and the bounds of
 *            keyframe 2; T_2w with S12 and the bounds of keyframe 1), both with pKF1's fx, fy, cx, cy as the reference takes them.
 *            Pa = T_aw * P under rot_kind; Pb = S_ba * Pa under sim_kind; (double)Pb[2] < 0.0 skips;
 *            invz = 1.0f / Pb[2] (the reference's 1.0 / z in double, narrowed to float, equals the float quotient: a double holds more than
 *            twice a float's digits); x = Pb[0] * invz, y = Pb[1] * invz; u = fx * x + cx, v = fy * y + cy: a product and then a sum,
 *            never an FMA.  This caller multiplies by invz, as :534 does, where :427 and fuse divide by z.
 *            IsInImage of the target, half-open; dist3D = sqrt(sum3(Pb[k]^2)): the norm in the target's camera frame, Ow is not read;
 *            dist3D < min_inv || dist3D > max_inv skips; there is no viewing-angle gate and the normal is not read;
 *            level from max_dist / dist3D (PredictScale divides mfMaxDistance, the table's max_dist); r = th * scale_factors[level];
 *            query as for fuse.
 * A slot at or beyond nslots[b] is a skipped row.  Whole rows are written and compare bit for bit.
 *
 * d_nvalid[b] is the number of valid rows of item b (valid = 1; for a query, point >= 0).  A malformed item has d_nvalid[b] = -1 and a row
 * of skipped records: nslots[b] outside 0 .. mcap, or an index >= npoints among the row's first nslots[b].  All of it is checked on the
 * device before any of these values addresses memory.  nlevels is 1 .. 16.  nitems * mcap and the number of workgroups stay within INT_MAX.
 *
 * agree, for pair p with n1[p] keypoints in keyframe 1 and n2[p] in keyframe 2 (the rows of two orbx_fuse_search_device calls, [P][qcap]):
 *    vnMatch1[i1] = best_idx12[p][i1] if best_dist12[p][i1] <= th_high, else -1 (i1 < n1[p]); vnMatch2 likewise from the 21 blocks;
 *    match12[p][i1] = idx2 = vnMatch1[i1] when idx2 >= 0 && idx2 < n2[p] && vnMatch2[idx2] == i1, else -1; -1 at and beyond n1[p];
 *    nfound[p] = the number of i1 with match12[p][i1] >= 0: what SearchBySim3 returns.  The caller passes th_high = TH_HIGH = 100.
 * A malformed pair has nfound[p] = -1 and a row of -1: nfound12[p] or nfound21[p] negative, or n1[p] or n2[p] outside 0 .. qcap.  Every
 * idx2 is checked before it indexes.  Everything is integer work.
 *
 * A handle holds one stream and one event of its own; calls on one handle run one after the other on the device.  The result does not
 * depend on scheduling: d_nvalid and nfound are integer counts. */
#ifndef ORBX_SIM3_H
#define ORBX_SIM3_H

#include <stddef.h>
#include <stdint.h>

#include "orbx.h"
#include "orbx_frustum.h"
#include "orbx_fuse.h"
#include "orbx_project.h"
#include "orbx_projmatch.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#define ORBX_SIM3_EXPORT __attribute__((visibility("default")))
#else
#define ORBX_SIM3_EXPORT
#endif

#define ORBX_SIM3_MATRIX 0
#define ORBX_SIM3_QUAT 1
#define ORBX_SIM3_PROJ_DIVIDE 0   /* SearchByProjection(pKF, Scw, vpPoints, vpMatched, ...), :427 */
#define ORBX_SIM3_PROJ_INVZ 1     /* ... with vpPointsKFs / vpMatchedKF, :534 */

typedef struct orbx_sim3 orbx_sim3;

/* One direction of a SearchBySim3 call, 176 bytes, 16-byte aligned. */
typedef struct orbx_sim3_item {
  float Raw[9];      /* the source keyframe's pose T_aw: row-major rotation */
  float taw[3];
  float qa[4];       /* x, y, z, w of T_aw.unit_quaternion() */
  float s;           /* the similarity S_ba: scale */
  float Rba[9];      /* its rotation matrix (unit), row-major */
  float tba[3];
  float qba[4];      /* x, y, z, w of its RxSO3's quaternion: NOT unit, squared norm s */
  float fx, fy, cx, cy;   /* pKF1's, for both directions */
  float bounds[4];   /* the target keyframe's {mnMinX, mnMinY, mnMaxX, mnMaxY} */
  float th;          /* the radius factor */
  float pad[2];
} orbx_sim3_item;

/* ORBX_E_INVALID for out = NULL or device < 0, ORBX_E_DEVICE when the device cannot be opened (reason: orbx_sim3_last_error(NULL)). */
ORBX_SIM3_EXPORT int orbx_sim3_create(orbx_sim3** out, int device);
ORBX_SIM3_EXPORT void orbx_sim3_destroy(orbx_sim3* p);
/* The reason of the handle's last failure; with p = NULL the calling thread's last failure of a call without a handle. */
ORBX_SIM3_EXPORT const char* orbx_sim3_last_error(const orbx_sim3* p);

/* The arguments the three emitters share:
 *   d_points  [npoints] orbx_frustum_point, 16-byte aligned
 *   d_items   [nitems] orbx_project_item (proj, fuse) or orbx_sim3_item (search)
 *   d_idx     [nitems][mcap] int32; d_nslots [nitems] int32
 *   d_out     [nitems][mcap] rows of the consumer, 16-byte aligned, OUT; d_nvalid [nitems] int32, OUT
 * The _device forms are asynchronous on `stream`; NULL is the handle's own stream.  ORBX_E_INVALID for what the host can check: NULL
 * arguments, sizes < 1, nlevels outside 1 .. 16, an unknown proj_kind, rot_kind, sum_order, sim_kind or log_kind, misaligned d_points or d_out,
 * nitems * mcap beyond INT_MAX, buffers on another device than the handle's, thresholds that are not finite, positive and strictly
 * increasing.  The forms without _device take host arrays of the same layout: they upload them, project, and return when the results are in
 * the caller's buffers.  The _reference forms are the host twins: the per-point loop in plain C++ on host arrays, libm's log called for
 * every point that reaches the level, no thresholds and no device; the same results, malformed items included, and ORBX_E_INVALID for a
 * log_scale_factor that is not finite and positive.  Reason of a twin's failure: orbx_sim3_last_error(NULL). */
ORBX_SIM3_EXPORT int orbx_sim3_proj_device(orbx_sim3* p, const orbx_frustum_point* d_points, int npoints, const orbx_project_item* d_items,
                                           int nitems, const int32_t* d_idx, const int32_t* d_nslots, int mcap, const float* thresholds,
                                           int nlevels, int proj_kind, int rot_kind, int sum_order, orbx_projmatch_point* d_out,
                                           int32_t* d_nvalid, void* stream);
ORBX_SIM3_EXPORT int orbx_sim3_proj(orbx_sim3* p, const orbx_frustum_point* points, int npoints, const orbx_project_item* items, int nitems,
                                    const int32_t* idx, const int32_t* nslots, int mcap, const float* thresholds, int nlevels, int proj_kind,
                                    int rot_kind, int sum_order, orbx_projmatch_point* out, int32_t* nvalid);
ORBX_SIM3_EXPORT int orbx_sim3_proj_reference(const orbx_frustum_point* points, int npoints, const orbx_project_item* items, int nitems,
                                              const int32_t* idx, const int32_t* nslots, int mcap, float log_scale_factor, int nlevels,
                                              int log_kind, int proj_kind, int rot_kind, int sum_order, orbx_projmatch_point* out,
                                              int32_t* nvalid);

ORBX_SIM3_EXPORT int orbx_sim3_fuse_device(orbx_sim3* p, const orbx_frustum_point* d_points, int npoints, const orbx_project_item* d_items,
                                           int nitems, const int32_t* d_idx, const int32_t* d_nslots, int mcap, const float* thresholds,
                                           const float* scale_factors, int nlevels, int rot_kind, int sum_order, orbx_fuse_query* d_out,
                                           int32_t* d_nvalid, void* stream);
ORBX_SIM3_EXPORT int orbx_sim3_fuse(orbx_sim3* p, const orbx_frustum_point* points, int npoints, const orbx_project_item* items, int nitems,
                                    const int32_t* idx, const int32_t* nslots, int mcap, const float* thresholds, const float* scale_factors,
                                    int nlevels, int rot_kind, int sum_order, orbx_fuse_query* out, int32_t* nvalid);
ORBX_SIM3_EXPORT int orbx_sim3_fuse_reference(const orbx_frustum_point* points, int npoints, const orbx_project_item* items, int nitems,
                                              const int32_t* idx, const int32_t* nslots, int mcap, float log_scale_factor,
                                              const float* scale_factors, int nlevels, int log_kind, int rot_kind, int sum_order,
                                              orbx_fuse_query* out, int32_t* nvalid);

ORBX_SIM3_EXPORT int orbx_sim3_search_device(orbx_sim3* p, const orbx_frustum_point* d_points, int npoints, const orbx_sim3_item* d_items,
                                             int nitems, const int32_t* d_idx, const int32_t* d_nslots, int mcap, const float* thresholds,
                                             const float* scale_factors, int nlevels, int rot_kind, int sum_order, int sim_kind,
                                             orbx_fuse_query* d_out, int32_t* d_nvalid, void* stream);
ORBX_SIM3_EXPORT int orbx_sim3_search(orbx_sim3* p, const orbx_frustum_point* points, int npoints, const orbx_sim3_item* items, int nitems,
                                      const int32_t* idx, const int32_t* nslots, int mcap, const float* thresholds, const float* scale_factors,
                                      int nlevels, int rot_kind, int sum_order, int sim_kind, orbx_fuse_query* out, int32_t* nvalid);
ORBX_SIM3_EXPORT int orbx_sim3_search_reference(const orbx_frustum_point* points, int npoints, const orbx_sim3_item* items, int nitems,
                                                const int32_t* idx, const int32_t* nslots, int mcap, float log_scale_factor,
                                                const float* scale_factors, int nlevels, int log_kind, int rot_kind, int sum_order,
                                                int sim_kind, orbx_fuse_query* out, int32_t* nvalid);

/* The agreement pass for pairs [0, npairs):
 *   d_best_idx12, d_best_dist12 [npairs][qcap] int32, d_nfound12 [npairs] int32: the search of direction 1 -> 2 (row p indexed by the
 *                keypoints of keyframe 1), as orbx_fuse_search_device wrote them; the 21 blocks likewise for direction 2 -> 1
 *   d_n1, d_n2   [npairs] int32: the keypoint counts N1 and N2 of the pair's keyframes
 *   d_match12    [npairs][qcap] int32, OUT; d_nfound [npairs] int32, OUT
 * ORBX_E_INVALID: NULL arguments, sizes < 1, npairs * qcap beyond INT_MAX, buffers on another device than the handle's. */
ORBX_SIM3_EXPORT int orbx_sim3_agree_device(orbx_sim3* p, const int32_t* d_best_idx12, const int32_t* d_best_dist12, const int32_t* d_nfound12,
                                            const int32_t* d_best_idx21, const int32_t* d_best_dist21, const int32_t* d_nfound21,
                                            const int32_t* d_n1, const int32_t* d_n2, int npairs, int qcap, int th_high, int32_t* d_match12,
                                            int32_t* d_nfound, void* stream);
ORBX_SIM3_EXPORT int orbx_sim3_agree(orbx_sim3* p, const int32_t* best_idx12, const int32_t* best_dist12, const int32_t* nfound12,
                                     const int32_t* best_idx21, const int32_t* best_dist21, const int32_t* nfound21, const int32_t* n1,
                                     const int32_t* n2, int npairs, int qcap, int th_high, int32_t* match12, int32_t* nfound);
ORBX_SIM3_EXPORT int orbx_sim3_agree_reference(const int32_t* best_idx12, const int32_t* best_dist12, const int32_t* nfound12,
                                               const int32_t* best_idx21, const int32_t* best_dist21, const int32_t* nfound21,
                                               const int32_t* n1, const int32_t* n2, int npairs, int qcap, int th_high, int32_t* match12,
                                               int32_t* nfound);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_SIM3_H */
