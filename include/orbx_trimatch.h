/* orbx_trimatch.h — the batched SearchForTriangulation: ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:907-1146) for P (keyframe,
 * keyframe) pairs at once, on the descriptors, keypoints and FeatureVectors a batch extraction and orbx_bow_transform_batch_device left in
 * HBM.  LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:466) calls the routine once per new keyframe against each of its 10 - 20
 * covisible neighbours: that is the batch.  Not part of the drop-in boundary (include/orbx.h): these entry points live in
 * liborbx_trimatch.so.  The library reads plain device arrays only; it takes nothing from a context or a vocabulary.
 *
 * In scope: the single-camera branch (!pKF1->mpCamera2 && !pKF2->mpCamera2, NLeft == -1) with Pinhole::epipolarConstrain
 * (src/CameraModels/Pinhole.cpp:107-129), bOnlyStereo, bCoarse and mbCheckOrientation.
 * Out of scope: two-camera rigs (the Tll / Tlr / Trl / Trr branch); KannalaBrandt8::epipolarConstrain, which triangulates (DESIGN.md
 * section 8 excludes that geometry); builds of the reference whose compiler contracts the gates' float expressions into FMAs.
 *
 * The specification is the reference's loop.  For pair p = (ia, ib), side A is pKF1 (the queries), side B is pKF2 (the candidates):
 *   walk the two FeatureVectors' ascending node lists; a node present on both sides is processed;
 *   for every A feature of the node, in fv_feat order: skip it when it has a point, and under only_stereo when it is not stereo
 *     (stereo: uright >= 0);
 *   its candidates are the B features of the node in fv_feat order; a candidate that has a point is skipped, and under only_stereo one that
 *     is not stereo;
 *   a remaining candidate competes when all three hold:
 *     (1) dist <= 50 (the Hamming distance of the two descriptors);
 *     (2) the epipole gate, only when neither feature is stereo: with distex = ep.x - x2, distey = ep.y - y2 the candidate is out when
 *         distex*distex + distey*distey < 100*scale_factor[octave2]: float32, every operation rounded, nothing contracted, the right-hand
 *         side one float multiplication;
 *     (3) the epipolar gate: `coarse` is set, or, literally Pinhole.cpp:115-128, all in float32 and evaluated left to right,
 *           a = x1*F00 + y1*F10 + F20,  b = x1*F01 + y1*F11 + F21,  c = x1*F02 + y1*F12 + F22,
 *           num = a*x2 + b*y2 + c,  den = a*a + b*b;  den == 0 fails;  dsqr = num*num/den;
 *         the candidate passes iff (double)dsqr < 3.84 * (double)level_sigma2[octave2]: a comparison of doubles, the literal is a double;
 *   NaNs and infinities in d_geom behave as C evaluates these expressions;
 *   the winner is the competing candidate of the smallest distance, the LAST of them in list order on a tie (:1017, dist > bestDist skips,
 *     so an equal distance replaces).  The reference's running bestDist only ever skips candidates that cannot win and the gates keep no
 *     state, so "argmin over the competing candidates, last wins" is the same function;
 *   with check_orientation: rot = angleA - angleB, + 360.0f when negative, bin = (int)round(rot * (1.0f / 30)), bin 30 -> 0; after the last
 *     node ComputeThreeMaxima (src/ORBmatcher.cc:2012-2053) over the 30 bin sizes; the matches of every other bin are removed.
 * (x1, y1) and (x2, y2) are the keypoints' x and y (mvKeysUn), octave2 the B keypoint's octave.
 *
 * Why everything is parallel: vbMatched2 is read (:1004) and never written, so no query depends on another; the rotation filter needs the
 * bin SIZES (integer counts) and each match's own bin.  The result does not depend on scheduling.
 *
 * Who computes the geometry: the CALLER, once per pair, as :914-920 and Pinhole.cpp:109-112 do, with its own Eigen:
 *   F12 = K1.transpose().inverse() * hat(t12) * R12 * K2.inverse() and ep = pKF2->mpCamera->project(T2w * Cw).
 * The reference recomputes the same F12 for every candidate; the library never forms it, so its rounding is the caller's.
 *
 * Precondition: no feature index occurs twice in a frame's fv_feat (orbx_bow_transform_batch_device guarantees it).  Breaking it leaves
 * the winner of a doubly listed query unspecified, but nothing is read or written out of bounds.
 *
 * A handle holds scratch memory, one stream and one event of its own; calls on one handle run one after the other on the device.
 * Environment, read at orbx_trimatch_create (results do not change): ORBX_TRIMATCH_LDS = the largest LDS block in bytes a call may stage a
 * pair in (0 .. 155648; pairs that need more run on global memory). */
#ifndef ORBX_TRIMATCH_H
#define ORBX_TRIMATCH_H

#include <stddef.h>
#include <stdint.h>

#include "orbx.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#define ORBX_TRIMATCH_EXPORT __attribute__((visibility("default")))
#else
#define ORBX_TRIMATCH_EXPORT
#endif

#define ORBX_TRIMATCH_MAX_LEVELS 16
#define ORBX_TRIMATCH_MAX_CAPACITY 65536   /* a candidate's position in its node's list takes 16 bits of the winner's key */

typedef struct orbx_trimatch orbx_trimatch;

/* One side of the pairs: a batch of keyframes at fixed stride.  The FeatureVector arrays are those orbx_bow_transform_batch_device writes. */
typedef struct orbx_trimatch_side {
  const orbx_keypoint* d_kps;   /* [nframes][capacity]; x, y, octave (side B) and angle (check_orientation) are read */
  const uint8_t* d_desc;        /* [nframes][capacity][32] */
  const int32_t* d_counts;      /* [nframes][2]: {keypoints, -} */
  const uint32_t* d_fv_node;    /* [nframes][capacity] */
  const int32_t* d_fv_ptr;      /* [nframes][capacity + 1] */
  const uint32_t* d_fv_feat;    /* [nframes][capacity] */
  const int32_t* d_fv_n;        /* [nframes] */
  const uint8_t* d_has_point;   /* [nframes][capacity], or NULL: no feature has a MapPoint.  Nonzero: on side A no query, on side B no candidate */
  const float* d_uright;        /* [nframes][capacity], or NULL: monocular (every value negative).  mvuRight: stereo means uright >= 0 */
  int nframes, capacity;
} orbx_trimatch_side;

/* ORBX_E_INVALID for out = NULL or device < 0, ORBX_E_DEVICE when the device cannot be opened (reason: orbx_trimatch_last_error(NULL)). */
ORBX_TRIMATCH_EXPORT int orbx_trimatch_create(orbx_trimatch** out, int device);
ORBX_TRIMATCH_EXPORT void orbx_trimatch_destroy(orbx_trimatch* m);
/* The reason of the handle's last failure; with m = NULL the calling thread's last orbx_trimatch_create failure. */
ORBX_TRIMATCH_EXPORT const char* orbx_trimatch_last_error(const orbx_trimatch* m);

/* SearchForTriangulation for pairs [0, npairs): d_pairs [npairs][2] int32 = {keyframe of a, keyframe of b}; a and b may be the same batch.
 *   d_geom [npairs][12] float32    F12 row-major (9 values), the epipole ep.x, ep.y, one pad value (not read)
 *   scale_factor, level_sigma2     [nlevels] float32 in HOST memory: mvScaleFactors and mvLevelSigma2 of side B's extractor; they are read
 *                                  during the call, 1 <= nlevels <= 16
 *   d_matches12 [npairs][a.capacity] int32   vMatches12: the B feature matched to A feature i, -1 for none.  vMatchedPairs is its
 *                                  non-negative entries in ascending i.  Several A features may name one B feature: no inverse is offered
 *   d_nmatches  [npairs] int32     the reference's return value
 * Whole rows are written (-1 past the frame's count).  d_nmatches[p] = -1 with a row of -1 for a malformed pair: a frame index outside its
 * batch, a count outside 0 .. capacity, a negative fv_n, an fv_feat entry that is not below its frame's count, or a B feature listed in
 * frame ib's fv_feat (every one of them is read as a candidate of some pair) whose octave lies outside [0, nlevels): checked on the device
 * before any index addresses memory, nothing is read past `capacity`.  Asynchronous on `stream`; NULL is the handle's own stream.
 * ORBX_E_INVALID for what the host can check: NULL arguments, sizes < 1, a capacity above 65536, nlevels outside 1 .. 16,
 * npairs * capacity beyond INT_MAX, buffers on another device than the handle's. */
ORBX_TRIMATCH_EXPORT int orbx_trimatch_pairs_device(orbx_trimatch* m, const orbx_trimatch_side* a, const orbx_trimatch_side* b,
                                                    const int32_t* d_pairs, int npairs, const float* d_geom, const float* scale_factor,
                                                    const float* level_sigma2, int nlevels, int only_stereo, int coarse,
                                                    int check_orientation, int32_t* d_matches12, int32_t* d_nmatches, void* stream);

/* The same call on host arrays of the same fixed-stride layout (the d_ members of a and b, pairs, geom and the results are host pointers
 * here); returns when the results are in the caller's buffers. */
ORBX_TRIMATCH_EXPORT int orbx_trimatch_pairs(orbx_trimatch* m, const orbx_trimatch_side* a, const orbx_trimatch_side* b, const int32_t* pairs,
                                             int npairs, const float* geom, const float* scale_factor, const float* level_sigma2, int nlevels,
                                             int only_stereo, int coarse, int check_orientation, int32_t* matches12, int32_t* nmatches);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_TRIMATCH_H */
