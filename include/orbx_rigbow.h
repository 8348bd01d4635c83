/* orbx_rigbow.h — the two-camera rig block of SearchByBoW, batched, and the stacked rig frame it runs on: ORBmatcher::SearchByBoW(KeyFrame*,
 * Frame&, ...) with F.Nleft != -1 (src/ORBmatcher.cc:223-425: the branch at :296-323 and the second accept block at :357-386) and
 * SearchByBoW(KeyFrame*, KeyFrame*, ...) with NLeft != -1 (:765-905, the gates at :800 and :820), for P (frame, frame) pairs at once.  Not
 * part of the drop-in boundary (include/orbx.h): these entry points live in liborbx_rigbow.so.  The library reads plain device arrays only;
 * it takes nothing from a context or a vocabulary.  The single-camera branches are include/orbx_match.h's; with every nleft = -1 entry 2
 * computes exactly what orbx_match_bow_pairs_device computes.
 *
 * Entry 1, orbx_rigbow_stack_device: from the buffers a batched rig extraction (include/orbx_fisheye.h) leaves to the layout the
 * reference's Frame has when Nleft != -1: mDescriptors is the left descriptors followed by the right ones (src/Frame.cc, cv::vconcat), and
 * right keypoint j has feature index Nleft + j.  For frame f, nl = counts_l[f][0], nr = counts_r[f][0]:
 *   d_kps_s  [F][cap_s]      rows 0 .. nl are the left keypoints, rows nl .. nl + nr the right ones (contiguous: nl + j, not cap_l + j,
 *                            because a FeatureVector must carry the reference's indices); rows from nl + nr on are zero
 *   d_desc_s [F][cap_s][32]  the same order; zero from nl + nr on
 *   d_counts_s [F][2] = {nl + nr, 0},  d_nleft [F] = nl
 * A frame is malformed when nl is outside 0 .. cap_l, nr outside 0 .. cap_r or nl + nr > cap_s: it gets counts_s = {-1, 0}, nleft = -1 and
 * zero rows, and nothing of it is read.  One launch for all frames, the sizes read on the device; descriptors move in 16-byte pieces,
 * keypoints (28-byte records that land at nl + j) in 4-byte words.
 * The stacked buffers are what orbx_bow_transform_batch_device takes (it answers a negative count with bow_n = fv_n = -1): the rig frame's
 * BowVector and FeatureVector are that call on them, unchanged -- the weights are added in feature order, left first, as Frame::ComputeBoW
 * does on mDescriptors.
 *
 * Entry 2, orbx_rigbow_pairs_device.  A side is orbx_match_side's fields and d_nleft [nframes]: Nleft of each stacked frame, -1 for a
 * single-camera frame (every feature is "left").  For pair p = (ia, ib), side A holds the queries (the keyframe), side B the features
 * that are taken.  nlA = nleft of A's frame, nlB of B's.
 *   Common nodes of the two FeatureVectors are processed in ascending order; within a node the A features whose valid flag is not 0, in
 *   fv_feat order.
 * ORBX_RIGBOW_FRAME (:223-425).  A features at indices >= nlA are ordinary queries (the reference reads their angle from mvKeysRight: the
 * stacked keypoint row).  b.d_valid is ignored.  For each query:
 *   scan the node's B features in fv_feat order, passing over the slots an earlier query took (both accepts below see the same snapshot);
 *   over candidates with idx < nlB (all of them when nlB = -1): bestDist1 / bestIdxF / bestDist2, strict `<` and
 *     `else if (dist < bestDist2)`, both from 256;
 *   over candidates with idx >= nlB: bestDist1R / bestIdxFR, strict `<` from 256 (bestDist2R is dead: the ratio test at :359 is `|| true`);
 *   if bestDist1 <= 50:
 *     when (float)bestDist1 < nn_ratio * (float)bestDist2 (one float multiplication, not contracted): slot bestIdxF takes the query,
 *       nmatches++;
 *     independently of that ratio test, when bestDist1R <= 50: slot bestIdxFR takes the query, nmatches++;
 *   if bestDist1 > 50 nothing is bound: also when there is no left candidate at all, and even with a right candidate at distance 0.
 *   One A feature may so hold two B slots.
 * ORBX_RIGBOW_KEYFRAMES (:765-905).  When nlA != -1, A features >= nlA are not queries (:800); when nlB != -1, B features >= nlB are not
 * candidates (:820); B features with valid 0 are no candidates; the accept is bestDist1 < 50 and the ratio test; one slot per query.
 * Rotation (check_orientation).  Every bound B slot leaves one histogram entry from angleA[query] - angleB[slot] on the stacked keypoints:
 * rot + 360.0f when negative, bin = (int)round(rot * (1.0f / 30)), bin 30 -> 0.  A query may leave two entries, in different bins.  After
 * the last node ComputeThreeMaxima (:2012-2053) over the 30 bin sizes; every entry of another bin clears its own slot, nmatches--.
 *
 * Why P pairs and the features of one pair can be processed in parallel without changing a result (include/orbx_match.h's argument holds):
 *   1. A stacked feature sits in exactly one node of its frame's FeatureVector, left or right.  The "taken slot" dependence -- both
 *      cameras' -- therefore never crosses a node: the chains of different nodes are independent; only the queries inside one node are
 *      sequential, and inside one query both accepts read the snapshot before either binds.
 *   2. The rotation filter needs the bin SIZES (integer counts) and each bound slot's own bin (its holder's angle and its own).
 * So the result does not depend on scheduling.
 * Precondition: no feature index occurs twice in a frame's fv_feat (orbx_bow_transform_batch_device guarantees it).  Breaking it leaves the
 * winner of colliding bindings unspecified, but nothing is read or written out of bounds.
 *
 * A handle holds scratch memory, one stream and one event of its own; calls on one handle run one after the other on the device.
 * Environment, read at orbx_rigbow_create (results do not change): ORBX_RIGBOW_LDS = the largest LDS block in bytes a workgroup may stage a
 * pair in (0 .. 155648; pairs that need more run on global memory), ORBX_RIGBOW_WAVE_NODE = the largest number of B candidates of a node a
 * wave keeps in registers (0 .. 64; larger nodes run the trip loop).  The LDS block holds B alone -- 40 bytes per B feature and 8 per
 * common node: 40 b.capacity + 8 min(a.capacity, b.capacity), capacities up to 65 535; A is read where it lies. */
#ifndef ORBX_RIGBOW_H
#define ORBX_RIGBOW_H

#include <stddef.h>
#include <stdint.h>

#include "orbx.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#define ORBX_RIGBOW_EXPORT __attribute__((visibility("default")))
#else
#define ORBX_RIGBOW_EXPORT
#endif

#define ORBX_RIGBOW_FRAME 0       /* :223-425 */
#define ORBX_RIGBOW_KEYFRAMES 1   /* :765-905 */

typedef struct orbx_rigbow orbx_rigbow;

/* Entry 1's input: the two extractions of F rig frames at fixed strides (the field meanings of orbx_rigmatch_side). */
typedef struct orbx_rigbow_rig {
  const orbx_keypoint* d_kps_l;   /* [nframes][cap_l] (mvKeys) */
  const uint8_t* d_desc_l;        /* [nframes][cap_l][32], 16-byte aligned */
  const int32_t* d_counts_l;      /* [nframes][2]: {keypoints, -} */
  const orbx_keypoint* d_kps_r;   /* [nframes][cap_r] (mvKeysRight) */
  const uint8_t* d_desc_r;        /* [nframes][cap_r][32], 16-byte aligned */
  const int32_t* d_counts_r;      /* [nframes][2] */
  int nframes, cap_l, cap_r;
} orbx_rigbow_rig;

/* Entry 2's side: a batch of stacked frames at fixed stride.  The FeatureVector arrays are those orbx_bow_transform_batch_device writes. */
typedef struct orbx_rigbow_side {
  const orbx_keypoint* d_kps;   /* [nframes][capacity]; the angle field is read (check_orientation) */
  const uint8_t* d_desc;        /* [nframes][capacity][32], 16-byte aligned */
  const int32_t* d_counts;      /* [nframes][2]: {features, -} */
  const uint32_t* d_fv_node;    /* [nframes][capacity] */
  const int32_t* d_fv_ptr;      /* [nframes][capacity + 1] */
  const uint32_t* d_fv_feat;    /* [nframes][capacity] */
  const int32_t* d_fv_n;        /* [nframes] */
  const uint8_t* d_valid;       /* [nframes][capacity], or NULL: every feature is valid */
  const int32_t* d_nleft;       /* [nframes]: Nleft, -1 for a single-camera frame; NULL: every frame is single-camera */
  int nframes, capacity;
} orbx_rigbow_side;

/* ORBX_E_INVALID for out = NULL or device < 0, ORBX_E_DEVICE when the device cannot be opened (reason: orbx_rigbow_last_error(NULL)). */
ORBX_RIGBOW_EXPORT int orbx_rigbow_create(orbx_rigbow** out, int device);
ORBX_RIGBOW_EXPORT void orbx_rigbow_destroy(orbx_rigbow* m);
/* The reason of the handle's last failure; with m = NULL the calling thread's last orbx_rigbow_create failure. */
ORBX_RIGBOW_EXPORT const char* orbx_rigbow_last_error(const orbx_rigbow* m);

/* Entry 1.  d_desc_s is 16-byte aligned.  Asynchronous on `stream`; NULL is the handle's own stream.  ORBX_E_INVALID for what the host can
 * check: NULL arguments, sizes < 1, nframes * a capacity beyond INT_MAX, buffers on another device than the handle's. */
ORBX_RIGBOW_EXPORT int orbx_rigbow_stack_device(orbx_rigbow* m, const orbx_rigbow_rig* rig, int cap_s, orbx_keypoint* d_kps_s, uint8_t* d_desc_s,
                                                int32_t* d_counts_s, int32_t* d_nleft, void* stream);

/* Entry 2 for pairs [0, npairs): d_pairs [npairs][2] int32 = {frame of a, frame of b}; a and b may be the same batch.
 *   d_match_b2a [npairs][b.capacity] int32      the A feature left in B slot i, -1 for none (the order of the reference's vpMapPointMatches)
 *   d_match_a2b [npairs][a.capacity][2] int32   {the B slot below nlB, the B slot from nlB on} A feature i holds, -1 for none; the second
 *                                               is always -1 in keyframes mode and when nlB = -1
 *   d_nmatches  [npairs] int32                  the reference's return value
 * Either match array may be NULL, not both.  Whole rows are written (-1 past the frame's count).  d_nmatches[p] = -1 with both rows all -1
 * when a frame index of the pair is outside its batch, a frame has a negative count or a negative fv_n, a fv_feat entry is not below its
 * frame's count, or a frame's nleft is outside [-1, count]: checked on the device, nothing is read past `capacity`.  Asynchronous on
 * `stream`; NULL is the handle's own stream.  ORBX_E_INVALID for what the host can check: NULL arguments, sizes < 1, an unknown mode,
 * 2 * npairs * capacity beyond INT_MAX, buffers on another device than the handle's. */
ORBX_RIGBOW_EXPORT int orbx_rigbow_pairs_device(orbx_rigbow* m, const orbx_rigbow_side* a, const orbx_rigbow_side* b, const int32_t* d_pairs,
                                                int npairs, int mode, float nn_ratio, int check_orientation, int32_t* d_match_b2a,
                                                int32_t* d_match_a2b, int32_t* d_nmatches, void* stream);

/* The same call on host arrays of the same fixed-stride layout (the d_ members of a and b, pairs and the results are host pointers here);
 * returns when the results are in the caller's buffers. */
ORBX_RIGBOW_EXPORT int orbx_rigbow_pairs(orbx_rigbow* m, const orbx_rigbow_side* a, const orbx_rigbow_side* b, const int32_t* pairs, int npairs,
                                         int mode, float nn_ratio, int check_orientation, int32_t* match_b2a, int32_t* match_a2b,
                                         int32_t* nmatches);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_RIGBOW_H */
