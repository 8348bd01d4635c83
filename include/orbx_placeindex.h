/* orbx_placeindex.h — place recognition through an inverted file that lives on the device and grows: the candidates of
 * orbx_place_query_device (include/orbx_place.h: the same arguments, the same outputs, the same rules for malformed input, the same
 * d_kf_score update, BIT-IDENTICAL results), with the membership step done the way KeyFrameDatabase does it -- a walk over
 * mvInvertedFile[word] for the query's words alone (src/KeyFrameDatabase.cc:617-640, :745-760) -- instead of a visit to every
 * (query, database row) pair.  The work of a query then goes with the postings its words touch, not with D.  These entry points live in
 * liborbx_placeindex.so, which like liborbx_place.so needs no vocabulary and no context, only a device.
 *
 * The database is the caller's: the orbx_place_db arrays, which the caller appends to and erases from as the dense interface defines.
 *   sync    orbx_placeindex_sync_device rebuilds the file from `db` as it stands: a CSR by word over the rows with d_n >= 0 (ptr[n_words + 1]
 *           and the row of every posting), and keeps a snapshot of d_n[0 .. count) and of the count.  Three steps: a histogram with
 *           integer atomics, an exclusive scan over the words, a scatter through integer cursors.  The order inside a word's list is
 *           whatever the cursors give; no result depends on it.  The file takes 4 bytes a posting in a block sized count * stride.
 *   add     the caller appends rows to its arrays and raises db->count.  Rows [synced count, count) are the TAIL: a query visits them
 *           pair by pair, as the dense call visits every row; the next sync folds them in.  A handle that was never synced has a synced
 *           count of 0: every row is tail, and the call is the dense call.
 *   erase   the caller sets d_n[d] = -1.  A query reads the CURRENT d_n and skips the postings of a row that is erased now.
 *   stale   any other disagreement between the snapshot and the current d_n of an indexed row (a negative snapshot and a count now, two
 *           different counts), or db->count below the synced count, makes EVERY query malformed: d_ncand = -1 (and d_nmerge = -1), nothing
 *           written, nothing scored.  A stale answer is never returned.  What the snapshot cannot see is the caller's to keep: an indexed
 *           row's ids and values stay as they were at the sync (a changed row is erased and re-added as a new last row, as in the
 *           reference's database).
 * A query id >= n_words has no postings and matches nothing.  A database id >= n_words or a database count above the stride (seen by the
 * sync for the rows it indexes, by the query for the tail) makes every query malformed.
 *
 * The query: words[q][d] and first[q][d] are cleared, then counted by integer atomicAdd / atomicMin over the postings of each query word
 * (order-free), the tail pairs are intersected by a wave each, and from there on the call IS orbx_place_query_device: membership, the
 * threshold and the list order, then -- for the scored pairs alone -- the ordered L1 sum of the pair's common words in ascending word id
 * (the one place a float is added), the column scan and the selection.  Nothing depends on scheduling.
 *
 * A handle holds the file, scratch memory (10 arrays of nq * ndb words), one stream and one event of its own; calls on one handle run one
 * after the other on the device.  Test-only limits from the environment at orbx_placeindex_create; results never change:
 * ORBX_PLACE_LDS (0 .. 4096) lowers the number of entries up to which a query is staged in LDS by the pair passes,
 * ORBX_PLACEINDEX_SCAN_TILE (2 .. 2048) the words one workgroup scans, so that small n_words take one, two and three levels of the scan,
 * ORBX_PLACEINDEX_GROUP (1 .. 64, a power of two) the lanes that share one query word's list in the count pass. */
#ifndef ORBX_PLACEINDEX_H
#define ORBX_PLACEINDEX_H

#include <stddef.h>
#include <stdint.h>

#include "orbx.h"
#include "orbx_place.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#define ORBX_PLACEINDEX_EXPORT __attribute__((visibility("default")))
#else
#define ORBX_PLACEINDEX_EXPORT
#endif

#define ORBX_PLACEINDEX_MAX_WORDS (1 << 24)   /* ORBvoc has 971 815 words, a k = 10, L = 6 tree at most 10^6 */

typedef struct orbx_placeindex orbx_placeindex;

/* n_words: the vocabulary's word count, 1 .. ORBX_PLACEINDEX_MAX_WORDS; word ids are [0, n_words).  ORBX_E_INVALID for out = NULL,
 * device < 0 or n_words outside that range, ORBX_E_DEVICE when the device cannot be opened or the file's arrays cannot be allocated
 * (reason: orbx_placeindex_last_error(NULL)). */
ORBX_PLACEINDEX_EXPORT int orbx_placeindex_create(orbx_placeindex** out, int device, int n_words);
ORBX_PLACEINDEX_EXPORT void orbx_placeindex_destroy(orbx_placeindex* p);
/* The reason of the handle's last failure; with p = NULL the calling thread's last orbx_placeindex_create failure. */
ORBX_PLACEINDEX_EXPORT const char* orbx_placeindex_last_error(const orbx_placeindex* p);

/* Rebuilds the inverted file from db->d_ids, d_n, count and stride (the other members are not read) and takes the snapshot.
 * Asynchronous on `stream`; NULL is the handle's own stream.  ORBX_E_INVALID for NULL arguments or buffers, count or stride < 1, count *
 * stride beyond INT_MAX, buffers on another device than the handle's. */
ORBX_PLACEINDEX_EXPORT int orbx_placeindex_sync_device(orbx_placeindex* p, const orbx_place_db* db, void* stream);

/* orbx_place_query_device through the file: every argument, output and error as there (include/orbx_place.h), plus the rules above. */
ORBX_PLACEINDEX_EXPORT int orbx_placeindex_query_device(orbx_placeindex* p, int kind, int n_candidates, const orbx_place_db* db,
                                                        const orbx_place_queries* q, int ccap, int32_t* d_cand, int32_t* d_ncand,
                                                        int32_t* d_merge, int32_t* d_nmerge, int32_t* d_stats, void* stream);

/* orbx_place_query through the file, on host arrays: uploads them, syncs the file to the upload, queries, and returns when the results
 * are in the caller's buffers.  The host sees everything: a database id >= n_words returns ORBX_E_INVALID like the malformed input
 * listed in orbx_place.h, with nothing written.  The file it built indexed the upload, not the caller's device arrays: the handle is left
 * unsynced (a synced count of 0). */
ORBX_PLACEINDEX_EXPORT int orbx_placeindex_query(orbx_placeindex* p, int kind, int n_candidates, const orbx_place_db* db,
                                                 const orbx_place_queries* q, int ccap, int32_t* cand, int32_t* ncand, int32_t* merge,
                                                 int32_t* nmerge, int32_t* stats);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_PLACEINDEX_H */
