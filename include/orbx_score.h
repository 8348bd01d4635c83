/* orbx_score.h — all six DBoW2 scorings (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp) for every (query, database) pair of two batches of
 * BowVectors.  TemplatedVocabulary::score (TemplatedVocabulary.h:162) calls the scoring object its header line names; every other score of
 * this project (orbx_bow_score_l1, orbx_kfdb_score, ORBVocabulary::score, orbx_bow_score_matrix_device) is L1Scoring::score whatever that
 * line says.  Not part of the drop-in boundary (include/orbx.h): these entry points live in liborbx_score.so.  The library needs no
 * vocabulary and no context, only a device: the scoring is an argument of every call, DBoW2's ScoringType values (ORBX_SCORE_*).  The
 * vectors must carry the norm the scoring demands (L1 for L1_NORM, CHI_SQUARE, KL and BHATTACHARYYA, L2 for L2_NORM, none for
 * DOT_PRODUCT): orbx_bow_finalize and orbx_bow_transform_batch_device give a vocabulary's vectors that norm.
 *
 * The specification is ScoringObject.cpp, restated as C in orbx_score_pair.  A vector is n entries (id ascending and unique, value); the
 * common words of the two vectors are visited in ascending id, `score` starts from 0 and every operation is rounded once (no FMA):
 *   L1_NORM        :23-68    score += fabs(vi - wi) - fabs(vi) - fabs(wi)                      result -score / 2.0
 *   L2_NORM        :73-120   score += vi * wi                                                  result score >= 1 ? 1.0 : 1.0 - sqrt(1.0 - score)
 *   CHI_SQUARE     :125-170  if (vi + wi != 0.0) score += vi * wi / (vi + wi)                  result 2. * score
 *   KL             :175-221  common: if (vi != 0 && wi != 0) score += vi * log(vi / wi); a word of the first vector alone adds
 *                            vi * (log(vi) - LOG_EPS) -- in the walk without a test, in the tail loop (the second vector is used up)
 *                            only when vi != 0                                                 result score
 *   BHATTACHARYYA  :226-266  score += sqrt(vi * wi)                                            result score
 *   DOT_PRODUCT    :271-311  score += vi * wi                                                  result score
 * vi is the first vector's value (the query's), wi the second's.  NaNs and infinities come out as C evaluates these expressions (a
 * negative product under sqrt is a NaN); a NaN's payload and sign are not part of the contract.  An empty intersection gives -0.0 under
 * L1_NORM (-score / 2.0 with score = 0), as the reference does.
 *
 * KL is host only.  vi * log(vi / wi) needs glibc's double log bit for bit, and the device has no restatement of it that could be held to
 * that: orbx_score_matrix_device and orbx_score_matrix return ORBX_E_INVALID for ORBX_SCORE_KL and write nothing; orbx_score_pair is the
 * only form that computes it.  LOG_EPS is libm's run-time log(DBL_EPSILON), evaluated once when the library is loaded, as the
 * reference's static initialiser does (ScoringObject.cpp:18); the compiler's folded constant has the same bits (0xC04205966F2B4F12),
 * both were compared with the reference library's own KL score of a one-word vector against an empty one.
 *
 * A handle holds one stream, one event and the host form's device block; calls on one handle run one after the other on the device.
 * ORBX_SCORE_LDS (0 .. 4096) in the environment at orbx_score_create lowers the number of entries up to which a query is staged in LDS
 * (longer queries are read where they lie); results do not change. */
#ifndef ORBX_SCORE_H
#define ORBX_SCORE_H

#include <stddef.h>
#include <stdint.h>

#include "orbx.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#define ORBX_SCORE_EXPORT __attribute__((visibility("default")))
#else
#define ORBX_SCORE_EXPORT
#endif

/* DBoW2::ScoringType (TemplatedVocabulary.h:45-53) */
#define ORBX_SCORE_L1_NORM 0
#define ORBX_SCORE_L2_NORM 1
#define ORBX_SCORE_CHI_SQUARE 2
#define ORBX_SCORE_KL 3
#define ORBX_SCORE_BHATTACHARYYA 4
#define ORBX_SCORE_DOT_PRODUCT 5

typedef struct orbx_score orbx_score;

/* ORBX_E_INVALID for out = NULL or device < 0, ORBX_E_DEVICE when the device cannot be opened (reason: orbx_score_last_error(NULL)). */
ORBX_SCORE_EXPORT int orbx_score_create(orbx_score** out, int device);
ORBX_SCORE_EXPORT void orbx_score_destroy(orbx_score* s);
/* The reason of the handle's last failure; with s = NULL the calling thread's last orbx_score_create failure. */
ORBX_SCORE_EXPORT const char* orbx_score_last_error(const orbx_score* s);

/* The score of one pair on the host: the specification, and the only form of KL.  A negative n is an empty vector.  NaN for a scoring
 * outside 0 .. 5 and for a NULL array of a vector with n > 0. */
ORBX_SCORE_EXPORT double orbx_score_pair(int scoring, const uint32_t* ida, const double* va, int na, const uint32_t* idb, const double* vb,
                                         int nb);

/* Every (query, database) pair, both sides in the fixed-stride device layout of orbx_bow_transform_batch_device (vector i: d_*_ids +
 * i * stride, d_*_n[i] entries; a negative n is an empty vector, an n above the stride is taken as the stride): d_scores [nq][ndb] double,
 * each entry bit-identical to orbx_score_pair of the pair (a NaN where that is a NaN).  Asynchronous on `stream`; NULL is the handle's own.
 * ORBX_E_INVALID, with nothing written, for ORBX_SCORE_KL (see above), a scoring outside 0 .. 5, NULL arguments, nq or ndb < 1, a stride
 * < 1, nq * ndb beyond INT_MAX, buffers on another device than the handle's. */
ORBX_SCORE_EXPORT int orbx_score_matrix_device(orbx_score* s, int scoring, const uint32_t* d_q_ids, const double* d_q_vals,
                                               const int32_t* d_q_n, int nq, int q_stride, const uint32_t* d_db_ids, const double* d_db_vals,
                                               const int32_t* d_db_n, int ndb, int db_stride, double* d_scores, void* stream);

/* The same on host compact CSR (q_ptr [nq + 1], db_ptr [ndb + 1], as orbx_bow_score_matrix takes them); scores [nq][ndb] in host memory,
 * written when the call returns ORBX_OK.  ORBX_E_INVALID also for row pointers that begin below 0 or descend. */
ORBX_SCORE_EXPORT int orbx_score_matrix(orbx_score* s, int scoring, const int32_t* q_ptr, const uint32_t* q_ids, const double* q_vals, int nq,
                                        const int32_t* db_ptr, const uint32_t* db_ids, const double* db_vals, int ndb, double* scores);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_SCORE_H */
