/* orbx_bow.h — the batched bag of words: Frame::ComputeBoW (TemplatedVocabulary::transform(features, BowVector&, FeatureVector&, levelsup),
 * Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1194) for B frames at once on the descriptors a batch extraction, a replay block or a
 * gathered part left in HBM, and L1Scoring::score for every (query, database) pair of two such batches.  Not part of the drop-in boundary
 * (include/orbx.h): these entry points live in liborbx_bow.so, which links liborbx.so.
 *
 * How it reaches the tree: the library does NOT read the vocabulary's device arrays.  The descent of every descriptor slot is one call of the
 * product's orbx_bow_transform_device over all nframes * capacity rows; from orbx_internal.h it takes orbx::voc_device alone (the GPU the tree
 * lives on).  What decides a result byte besides the records — whether a word's weights are added (TF_IDF, TF) or the first one kept (IDF,
 * BINARY), and which norm divides the vector (L1, L2, none) — it learns at orbx_bow_create by running the product's own orbx_bow_finalize, the
 * specification of these results, on a three-feature probe.  Consequence: the four scorings whose vectors carry the L1 norm (L1_NORM,
 * CHI_SQUARE, KL, BHATTACHARYYA) look alike to this library; the score matrix rejects L2_NORM and DOT_PRODUCT vocabularies and computes
 * L1Scoring::score for the others.
 *
 * Per frame the results are byte-identical to orbx_bow_transform + orbx_bow_finalize (BowVector) and to ORBVocabulary::transform's
 * FeatureVector on the frame's first counts[f][0] descriptor rows.
 *
 * A handle holds scratch memory, one stream and one event of its own; it grows the scratch on the first call that needs more and allocates
 * nothing afterwards.  Calls on one handle run one after the other on the device (each waits for the previous one).  The vocabulary must
 * outlive the handle; the handle may be destroyed before the context.  ORBX_BOW_LDS (0 .. 4096) in the environment at orbx_bow_create lowers
 * the number of features up to which a frame is sorted in LDS (larger frames use global memory); results do not change. */
#ifndef ORBX_BOW_H
#define ORBX_BOW_H

#include <stddef.h>
#include <stdint.h>

#include "orbx.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#define ORBX_BOW_EXPORT __attribute__((visibility("default")))
#else
#define ORBX_BOW_EXPORT
#endif

typedef struct orbx_bow orbx_bow;

/* levelsup as in transform(): the FeatureVector's nodes are those at level L - levelsup (node 0 when that is <= 0).
 * ORBX_E_INVALID for a NULL or empty vocabulary or levelsup < 0 (reason: orbx_bow_last_error(NULL)). */
ORBX_BOW_EXPORT int orbx_bow_create(orbx_bow** out, orbx_voc* voc, int levelsup);
ORBX_BOW_EXPORT void orbx_bow_destroy(orbx_bow* b);
/* The reason of the handle's last failure; with b = NULL the calling thread's last orbx_bow_create failure. */
ORBX_BOW_EXPORT const char* orbx_bow_last_error(const orbx_bow* b);

/* transform() for frames [0, nframes).  d_desc [nframes][capacity][32] and d_counts [nframes][2] as orbx_extract_batch_device, a replay block
 * or a gathered part hold them; every descriptor row is read (rows past a frame's count may hold anything), nothing is written to them.
 *   d_bow_ids  [nframes][capacity] uint32   word ids, ascending          d_bow_vals [nframes][capacity] double
 *   d_bow_n    [nframes] int32              entries; -1 where the frame's count is negative (nothing else of that frame is written)
 *   d_fv_node  [nframes][capacity] uint32   distinct node ids at level L - levelsup, ascending
 *   d_fv_ptr   [nframes][capacity + 1] int32   node j's features are d_fv_feat[f][ptr[j] .. ptr[j + 1])
 *   d_fv_feat  [nframes][capacity] uint32   feature indices (positions in the frame), ascending inside a node
 *   d_fv_n     [nframes] int32              nodes; -1 as above
 * Slots past a frame's n are unspecified.  Either output group (the three d_bow_*, or the four d_fv_*) may be NULL as a whole and is then
 * skipped.  Asynchronous on `stream`; a NULL stream is the handle's own.  ORBX_E_INVALID for nframes < 1, capacity < 1, nframes * capacity
 * beyond INT_MAX, NULL inputs, a partly NULL or entirely missing output, or buffers on another device than the vocabulary. */
ORBX_BOW_EXPORT int orbx_bow_transform_batch_device(orbx_bow* b, const uint8_t* d_desc, const int32_t* d_counts, int nframes, int capacity,
                                                    uint32_t* d_bow_ids, double* d_bow_vals, int32_t* d_bow_n, uint32_t* d_fv_node,
                                                    int32_t* d_fv_ptr, uint32_t* d_fv_feat, int32_t* d_fv_n, void* stream);

/* Host convenience: host descriptors and counts in, compact CSR out; returns when the results are in the caller's buffers.
 *   bow_ptr [nframes + 1], bow_ids / bow_vals [bow_ptr[nframes]]: the layout orbx_bow_score_l1_batch takes as db_ptr / db_ids / db_vals
 *   fv_ptr [nframes + 1]: frame f's nodes are fv_node[fv_ptr[f] .. fv_ptr[f + 1]); fv_feat_ptr [fv_ptr[nframes] + 1]: node j's features are
 *   fv_feat[fv_feat_ptr[j] .. fv_feat_ptr[j + 1])
 * A frame with a negative count has empty rows.  Every array but the two row pointers must hold nframes * capacity entries (fv_feat_ptr one
 * more): no frame produces more than its capacity. */
ORBX_BOW_EXPORT int orbx_bow_transform_batch(orbx_bow* b, const uint8_t* desc, const int32_t* counts, int nframes, int capacity,
                                             int32_t* bow_ptr, uint32_t* bow_ids, double* bow_vals, int32_t* fv_ptr, uint32_t* fv_node,
                                             int32_t* fv_feat_ptr, uint32_t* fv_feat);

/* L1Scoring::score (ScoringObject.cpp:23-68) for every (query, database) pair, both sides in the fixed-stride device layout above (vector i:
 * d_*_ids + i * stride, d_*_n[i] entries, a negative n counts as empty): d_scores [nq][ndb] double, each entry bit-identical to
 * orbx_bow_score_l1 of the pair.  ORBX_E_INVALID for a vocabulary whose vectors do not carry the L1 norm.  Asynchronous on `stream`. */
ORBX_BOW_EXPORT int orbx_bow_score_matrix_device(orbx_bow* b, const uint32_t* d_q_ids, const double* d_q_vals, const int32_t* d_q_n, int nq,
                                                 int q_stride, const uint32_t* d_db_ids, const double* d_db_vals, const int32_t* d_db_n, int ndb,
                                                 int db_stride, double* d_scores, void* stream);
/* The same on host compact CSR (q_ptr [nq + 1], db_ptr [ndb + 1]); scores [nq][ndb] in host memory. */
ORBX_BOW_EXPORT int orbx_bow_score_matrix(orbx_bow* b, const int32_t* q_ptr, const uint32_t* q_ids, const double* q_vals, int nq,
                                          const int32_t* db_ptr, const uint32_t* db_ids, const double* db_vals, int ndb, double* scores);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_BOW_H */
