/* orbx_place.h — batched place recognition: KeyFrameDatabase::DetectRelocalizationCandidates (src/KeyFrameDatabase.cc:733-845, the call of
 * Tracking::Relocalization) and KeyFrameDatabase::DetectNBestCandidates (:604-730, the one Detect* routine LoopClosing.cc still calls,
 * :433) for Q query BowVectors against D keyframe BowVectors at once, on the vectors orbx_bow_transform_batch_device left in HBM.  It is
 * the step between BowBatch and MatchBatch / ProjMatchBatch: which keyframes each frame is to be matched against.  Not part of the drop-in
 * boundary (include/orbx.h): these entry points live in liborbx_place.so.  Like liborbx_score.so the library needs no vocabulary and no
 * context, only a device; it reads plain device arrays.
 *
 * The call's result is that of calling the reference routine Q times in order, query 0 first, on one database, with distinct query ids.
 * Rows are database rows in add() order (a re-added keyframe is a new last row, an erased row has the count -1 and shares a word with
 * nobody).  For query q:
 *   1. membership: words[d] = the number of word ids common to q and row d.  Row d is IN THE QUERY iff words[d] > 0 and d is not in q's
 *      exclusion row (:623-633, :748-754; spConnectedKF, N-best only).  The reference gives the query keyframe no mark of its own, so the
 *      library does not either: the caller keeps a query keyframe out of the database, as the reference's callers do.
 *   2. list order (lKFsSharingWords): ascending (lowest common word id, row).
 *   3. maxCommonWords = the largest words[d] in the query; minCommonWords = (int)(maxCommonWords * 0.8f), a float32 product, truncated.
 *   4. the rows in the query with words > minCommonWords are SCORED: si = (float)L1Scoring::score(q, d), the double bit-identical to
 *      orbx_score_pair(ORBX_SCORE_L1_NORM, ...) (common words in ascending id, every operation rounded once), then narrowed;
 *      kf_score[d] = si.
 *   5. covisibility accumulation, for each scored row i in list order (:675-700, :796-821): acc = best = si, holder = i; for each
 *      cov[i][k] >= 0 in order that is in the query, s2 = kf_score[that row] -- this query's score if the row was scored, otherwise what an
 *      earlier query of the call, or the array as it came in, left there --, acc += s2 in float32, and if s2 > best the holder becomes that
 *      row and best = s2.
 *   6. ORBX_PLACE_RELOC: bestAcc = the largest acc, from 0; minRetain = 0.75f * bestAcc; the candidates are, in list order, the holders
 *      with acc > minRetain and kf_map[holder] == q_map[q], the first occurrence of a holder (the map test comes first, :828-842).
 *   7. ORBX_PLACE_NBEST: a stable sort of (acc, holder) by acc descending (std::list::sort(compFirst): ties keep list order); walking it,
 *      a holder not seen yet goes to `cand` (vpLoopCand) if kf_map[holder] == q_map[q] and cand is short of n_candidates, otherwise to
 *      `merge` (vpMergeCand) if it is of another map and merge is short of n_candidates; it is seen either way.
 * Nothing depends on scheduling: no float atomic, every float sum in the reference's order.
 *
 * Out of scope:
 *   isBad() keyframes: the reference erases them from the database, and its N-best walk never advances past one (:712-713);
 *   a bad map in the merge test (:721);
 *   the mn*Query / mn*Words marks: membership is recomputed per query, which equals the reference for query ids that never repeat (the
 *   same keyframe id asked twice finds the first call's marks, :623-631: not restated here);
 *   a frame id of 0 against the KeyFrame constructor's mnRelocQuery(0);
 *   DetectLoopCandidates, DetectCandidates and DetectBestCandidates;
 *   scorings other than L1, which is what every score of this class is;
 *   acc values that are NaN: compFirst is no ordering of them.
 *
 * A handle holds scratch memory (10 arrays of nq * ndb words), one stream and one event of its own; calls on one handle run one after the
 * other on the device.  ORBX_PLACE_LDS (0 .. 4096) in the environment at orbx_place_create lowers the number of entries up to which a query
 * is staged in LDS (longer queries are read where they lie); results do not change. */
#ifndef ORBX_PLACE_H
#define ORBX_PLACE_H

#include <stddef.h>
#include <stdint.h>

#include "orbx.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#define ORBX_PLACE_EXPORT __attribute__((visibility("default")))
#else
#define ORBX_PLACE_EXPORT
#endif

#define ORBX_PLACE_RELOC 0   /* DetectRelocalizationCandidates: kf_score is mRelocScore */
#define ORBX_PLACE_NBEST 1   /* DetectNBestCandidates: kf_score is mPlaceRecognitionScore */
#define ORBX_PLACE_COV 10    /* GetBestCovisibilityKeyFrames(10) */

typedef struct orbx_place orbx_place;

/* The database: D keyframe BowVectors in the fixed-stride layout orbx_bow_transform_batch_device writes (row d: d_ids + d * stride,
 * ids ascending, d_n[d] entries; d_n[d] < 0: an erased row). */
typedef struct orbx_place_db {
  const uint32_t* d_ids;      /* [count][stride] */
  const double* d_vals;       /* [count][stride] */
  const int32_t* d_n;         /* [count] */
  const int32_t* d_kf_map;    /* [count]: the id of the keyframe's map */
  const int32_t* d_kf_cov;    /* [count][10]: GetBestCovisibilityKeyFrames(10) as rows, in that order, padded with -1 (any negative value) */
  float* d_kf_score;          /* [count], IN / OUT: mRelocScore / mPlaceRecognitionScore as the keyframe carries it into and out of the call */
  int count, stride;
} orbx_place_db;

/* The queries: Q BowVectors in the same layout (d_n[q] < 0: an empty query). */
typedef struct orbx_place_queries {
  const uint32_t* d_ids;      /* [count][stride] */
  const double* d_vals;       /* [count][stride] */
  const int32_t* d_n;         /* [count] */
  const int32_t* d_q_map;     /* [count]: the id of the query's map (pMap / pKF->GetMap()) */
  const int32_t* d_excl_ptr;  /* [count + 1], or NULL (no exclusions; always so for ORBX_PLACE_RELOC): row q of d_excl_idx */
  const int32_t* d_excl_idx;  /* [n_excl]: the excluded rows of each query (spConnectedKF), strictly ascending within a query */
  int count, stride, n_excl;
} orbx_place_queries;

/* ORBX_E_INVALID for out = NULL or device < 0, ORBX_E_DEVICE when the device cannot be opened (reason: orbx_place_last_error(NULL)). */
ORBX_PLACE_EXPORT int orbx_place_create(orbx_place** out, int device);
ORBX_PLACE_EXPORT void orbx_place_destroy(orbx_place* p);
/* The reason of the handle's last failure; with p = NULL the calling thread's last orbx_place_create failure. */
ORBX_PLACE_EXPORT const char* orbx_place_last_error(const orbx_place* p);

/* The candidates of queries [0, q->count):
 *   kind          ORBX_PLACE_RELOC or ORBX_PLACE_NBEST; n_candidates: nNumCandidates (N-best; not read for reloc)
 *   d_cand        [Q][ccap] int32, OUT: the candidate rows (reloc: vpRelocCandidates, N-best: vpLoopCand), -1 beyond the count
 *   d_ncand       [Q] int32, OUT: the full count, also when it exceeds ccap
 *   d_merge, d_nmerge  the same for vpMergeCand; ORBX_PLACE_NBEST only (NULL for reloc)
 *   d_stats       [Q][4] int32, OUT: {rows in the query, scored rows, maxCommonWords, minCommonWords}
 *   db->d_kf_score  updated: the last query of the call that scored a row leaves its si there
 * Malformed input the device checks before it addresses memory with it: a database count above the stride or a d_kf_cov entry >= D make
 * every query malformed; a query count above its stride, or an exclusion row that leaves [0, n_excl], holds an index outside [0, D) or
 * does not ascend strictly, make that query malformed.  A malformed query has d_ncand = -1 (and d_nmerge = -1); its rows of d_cand, d_merge
 * and d_stats stay untouched, and it scores nothing.
 * Asynchronous on `stream`; NULL is the handle's own stream.
 * ORBX_E_INVALID for what the host can check: NULL arguments, an unknown kind, counts, strides or ccap < 1, n_candidates < 1 for N-best,
 * n_excl < 0, exclusions or merge arrays given for reloc, merge arrays missing for N-best, Q * D beyond INT_MAX, buffers on another device
 * than the handle's. */
ORBX_PLACE_EXPORT int orbx_place_query_device(orbx_place* p, int kind, int n_candidates, const orbx_place_db* db, const orbx_place_queries* q,
                                              int ccap, int32_t* d_cand, int32_t* d_ncand, int32_t* d_merge, int32_t* d_nmerge,
                                              int32_t* d_stats, void* stream);

/* The same on host arrays of the same layout (the d_ members and the results are host pointers here): uploads them, queries, and returns
 * when the results are in the caller's buffers; kf_score is read and updated.  Here the host sees everything, so all malformed input
 * listed above returns ORBX_E_INVALID, with nothing written. */
ORBX_PLACE_EXPORT int orbx_place_query(orbx_place* p, int kind, int n_candidates, const orbx_place_db* db, const orbx_place_queries* q, int ccap,
                                       int32_t* cand, int32_t* ncand, int32_t* merge, int32_t* nmerge, int32_t* stats);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_PLACE_H */
