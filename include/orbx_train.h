/* orbx_train.h — vocabulary training: DBoW2's TemplatedVocabulary::create (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:558-616) with the
 * k-means of the large nodes on the GPU.  Offline work, not part of the per-frame product: it lives in liborbx_train.so, which links
 * liborbx.so and uses only the product ABI (include/orbx.h): the finished tree is an ordinary orbx_voc made by orbx_voc_create, and the IDF
 * pass sends every training descriptor through orbx_bow_transform.
 *
 * Contract: the result equals, node for node (parent, leaf flag, descriptor, weight bits), what the reference's create computes in a process
 * that ran DUtils::Random::SeedRandOnce(seed) and made no other rand() call before create.  The library restates glibc's srand / rand
 * (TYPE_3, random_r) and never touches the process's own random state.  Two defined departures:
 *   - an empty cluster during the Lloyd iterations (the reference dereferences a released cv::Mat there, FORB.cpp:31-35 then :94) keeps its
 *     previous centre; it still becomes a child node, and with fewer than two descriptors it is never recursed into;
 *   - a node that has not converged after max_iterations assignment passes fails with ORBX_E_NOCONVERGE (the reference loops forever).
 * The GPU k-means runs on the calling thread's current HIP device; ctx must live there too (orbx_create with device_id < 0 picks it). */
#ifndef ORBX_TRAIN_H
#define ORBX_TRAIN_H

#include <limits.h>
#include <stdint.h>

#include "orbx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ORBX_E_NOCONVERGE (-16)   /* a node's k-means did not converge within max_iterations (orbx_train_vocabulary) */

typedef struct orbx_train_params {
  int k, L;               /* branching factor 2..20, depth 1..10 */
  int weighting;          /* DBoW2::WeightingType: 0 TF_IDF, 1 TF, 2 IDF, 3 BINARY */
  int scoring;            /* DBoW2::ScoringType 0..5 */
  uint32_t seed;          /* = DUtils::Random::SeedRandOnce(seed) before create */
  int device_min_node;    /* k-means nodes with at least this many descriptors run on the GPU; < 0: the measured default
                             (ORBX_TRAIN_DEVICE_MIN_NODE); INT_MAX: host only; k + 1: every k-means node on the GPU */
  int max_iterations;     /* assignment passes per node (the first one included); 0: ORBX_TRAIN_MAX_ITERATIONS */
} orbx_train_params;

#define ORBX_TRAIN_DEVICE_MIN_NODE 4096
#define ORBX_TRAIN_MAX_ITERATIONS 10000

typedef struct orbx_train_stats {
  int device_nodes, host_nodes;   /* k-means nodes (more than k descriptors) run on each side */
  int64_t iterations;             /* assignment passes over all k-means nodes */
  int64_t empty_clusters;         /* clusters found empty when the means were computed (the first departure above) */
  double ms_device, ms_host;      /* k-means + partition of the GPU nodes (wall time, device transfers included) / of the host nodes */
  double ms_weights, ms_create;   /* the IDF pass (descent + counting) / the orbx_voc_create calls */
} orbx_train_stats;

/* desc: N = doc_offsets[ndocs] rows of 32 bytes; document d is rows [doc_offsets[d], doc_offsets[d+1]) (doc_offsets[0] = 0, non-decreasing),
 * in the order of create's vector<vector<cv::Mat>>.  *out receives a new vocabulary on ctx.  stats may be NULL. */
int orbx_train_vocabulary(orbx_ctx* ctx, const uint8_t* desc, const int64_t* doc_offsets, int ndocs, const orbx_train_params* p,
                          orbx_voc** out, orbx_train_stats* stats);

/* The message of this thread's last failed orbx_train_vocabulary ("" after a success). */
const char* orbx_train_last_error(void);

/* glibc's srand(seed) then n calls of rand(), into out[n]: the restatement the trainer draws from (test hook). */
int orbx_train_glibc_rand(uint32_t seed, int n, int32_t* out);

#ifdef __cplusplus
}
#endif
#endif  /* ORBX_TRAIN_H */
