/* orbx_match.h — the batched SearchByBoW: ORBmatcher::SearchByBoW (src/ORBmatcher.cc:223-425, KeyFrame against Frame, and :765-905, KeyFrame
 * against KeyFrame; the single-camera branches) for P (frame, frame) pairs at once, on the descriptors, keypoints and FeatureVectors a batch
 * extraction and orbx_bow_transform_batch_device left in HBM.  Not part of the drop-in boundary (include/orbx.h): these entry points live in
 * liborbx_match.so.  The library reads plain device arrays only; it takes nothing from a context or a vocabulary.
 * The two-camera rig branches (Nleft != -1) are include/orbx_rigbow.h's (liborbx_rigbow.so).
 *
 * The specification is the reference's loop.  For pair p = (ia, ib), side A holds the queries (the "keyframe"), side B the frame whose
 * features are taken:
 *   walk the two FeatureVectors' ascending node lists; a node present on both sides is processed, in ascending order;
 *   for every A feature of the node, in fv_feat order, whose valid flag is not 0: scan the B features of the node in fv_feat order, skipping
 *     those an earlier A feature matched (and, in keyframe mode, those whose valid flag is 0); keep bestDist1 (strict <: the first minimum in
 *     list order wins), bestIdx and bestDist2 (the second-smallest distance, ties included), both starting at 256;
 *   accept when bestDist1 <= 50 (ORBX_MATCH_FRAME) resp. bestDist1 < 50 (ORBX_MATCH_KEYFRAMES) and
 *     (float)bestDist1 < nn_ratio * (float)bestDist2 (one float multiplication, not contracted);
 *   with check_orientation: rot = angleA - angleB, + 360.0f when negative, bin = (int)round(rot * (1.0f / 30)), bin 30 -> 0; after the last
 *     node ComputeThreeMaxima (src/ORBmatcher.cc:2012-2053) over the 30 bin sizes; the matches of every other bin are removed.
 * In frame mode the result equals orbx_search_by_bow of the pair.
 *
 * Why P pairs and the features of one pair can be processed in parallel without changing a result:
 *   1. A feature sits in exactly one node of its frame's FeatureVector.  The "already matched" dependence therefore never crosses a node: the
 *      chains of different nodes are independent; only the A features inside one node are sequential.
 *   2. The rotation filter needs the bin SIZES (integer counts: the order of the additions does not matter) and each match's own bin.
 * So the result does not depend on scheduling.
 *
 * Precondition: no feature index occurs twice in a frame's fv_feat (orbx_bow_transform_batch_device guarantees it).  Breaking it leaves the
 * winner of colliding matches unspecified, but nothing is read or written out of bounds.
 *
 * A handle holds scratch memory, one stream and one event of its own; calls on one handle run one after the other on the device.
 * Environment, read at orbx_match_create (results do not change): ORBX_MATCH_LDS = the largest LDS block in bytes a call may stage a pair in
 * (0 .. 155648; pairs that need more run on global memory), ORBX_MATCH_WAVE_NODE = the largest number of B candidates of a node a wave keeps in
 * registers (0 .. 64; larger nodes run the trip loop). */
#ifndef ORBX_MATCH_H
#define ORBX_MATCH_H

#include <stddef.h>
#include <stdint.h>

#include "orbx.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#define ORBX_MATCH_EXPORT __attribute__((visibility("default")))
#else
#define ORBX_MATCH_EXPORT
#endif

#define ORBX_MATCH_FRAME 0       /* :223-425: bestDist1 <= 50; b.d_valid is ignored */
#define ORBX_MATCH_KEYFRAMES 1   /* :765-905: bestDist1 < 50; B features with valid 0 are no candidates */

typedef struct orbx_match orbx_match;

/* One side of the pairs: a batch of frames at fixed stride.  The FeatureVector arrays are those orbx_bow_transform_batch_device writes. */
typedef struct orbx_match_side {
  const orbx_keypoint* d_kps;   /* [nframes][capacity]; the angle field is read (check_orientation) */
  const uint8_t* d_desc;        /* [nframes][capacity][32] */
  const int32_t* d_counts;      /* [nframes][2]: {keypoints, -} */
  const uint32_t* d_fv_node;    /* [nframes][capacity] */
  const int32_t* d_fv_ptr;      /* [nframes][capacity + 1] */
  const uint32_t* d_fv_feat;    /* [nframes][capacity] */
  const int32_t* d_fv_n;        /* [nframes] */
  const uint8_t* d_valid;       /* [nframes][capacity], or NULL: every feature is valid */
  int nframes, capacity;
} orbx_match_side;

/* ORBX_E_INVALID for out = NULL or device < 0, ORBX_E_DEVICE when the device cannot be opened (reason: orbx_match_last_error(NULL)). */
ORBX_MATCH_EXPORT int orbx_match_create(orbx_match** out, int device);
ORBX_MATCH_EXPORT void orbx_match_destroy(orbx_match* m);
/* The reason of the handle's last failure; with m = NULL the calling thread's last orbx_match_create failure. */
ORBX_MATCH_EXPORT const char* orbx_match_last_error(const orbx_match* m);

/* SearchByBoW for pairs [0, npairs): d_pairs [npairs][2] int32 = {frame of a, frame of b}; a and b may be the same batch.
 *   d_match_b2a [npairs][b.capacity] int32   the A feature matched to B feature i, -1 for none (the reference's vpMapPointMatches order)
 *   d_match_a2b [npairs][a.capacity] int32   its inverse: matches are one to one
 *   d_nmatches  [npairs] int32               the reference's return value
 * Either match array may be NULL, not both.  Whole rows are written (-1 past the frame's count).  d_nmatches[p] = -1 with both rows all -1
 * when a frame index of the pair is outside its batch, a frame has a negative count or a negative fv_n, or a fv_feat entry is not below its
 * frame's count: checked on the device, nothing is read past `capacity`.  Asynchronous on `stream`; NULL is the handle's own stream.
 * ORBX_E_INVALID for what the host can check: NULL arguments, sizes < 1, an unknown mode, npairs * capacity beyond INT_MAX, buffers on
 * another device than the handle's. */
ORBX_MATCH_EXPORT int orbx_match_bow_pairs_device(orbx_match* m, const orbx_match_side* a, const orbx_match_side* b, const int32_t* d_pairs,
                                                  int npairs, int mode, float nn_ratio, int check_orientation, int32_t* d_match_b2a,
                                                  int32_t* d_match_a2b, int32_t* d_nmatches, void* stream);

/* The same call on host arrays of the same fixed-stride layout (the d_ members of a and b, pairs and the results are host pointers here);
 * returns when the results are in the caller's buffers. */
ORBX_MATCH_EXPORT int orbx_match_bow_pairs(orbx_match* m, const orbx_match_side* a, const orbx_match_side* b, const int32_t* pairs, int npairs,
                                           int mode, float nn_ratio, int check_orientation, int32_t* match_b2a, int32_t* match_a2b,
                                           int32_t* nmatches);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_MATCH_H */
