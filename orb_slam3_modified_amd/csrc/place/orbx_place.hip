// Batched place recognition (include/orbx_place.h): KeyFrameDatabase::DetectRelocalizationCandidates and DetectNBestCandidates
// (src/KeyFrameDatabase.cc:733-845, :604-730) for Q query BowVectors against D keyframe BowVectors.  Everything costly is independent of the
// score state the reference carries from one query to the next, so it runs for all Q x D pairs at once; the state itself is a scan down
// each database column, and no query waits for another.  Five launches a call:
//   k_place_check    a thread per database row: a count above the stride or a covisibility entry >= D sets the call's db_bad word
//   k_place_pairs    grid Q * ceil(D / 32), workgroups of 8 waves, A WAVE PER PAIR in the shape of csrc/score/orbx_score.hip's k_score: the
//                    query staged once per workgroup in LDS (side/orbx_bowvec_device.h; a query longer than the handle's limit is read
//                    where it lies), the wave's lanes stride over the database vector and binary-search the query.  The ballot of the hits
//                    is the compaction: its popcount is the common-word count, its first lane of the first stride with a hit holds the
//                    lowest common word, and the L1 terms are taken out of the hit lanes in ascending lane order and added to a sum that is
//                    uniform over the wave -- the reference's additions in its order.  Lane 0 stores {words, first word, (float)score}.
//   k_place_members  a workgroup per query: the device checks, membership (words > 0, not excluded), maxCommonWords, the threshold, the
//                    scored rows compacted in row order and then ranked by (first word, row) -- lKFsSharingWords' order restricted to
//                    lScoreAndMatch -- and the stats.
//   k_place_scan     a thread per database column, down the Q queries: `cur` starts as kf_score[d]; a query that scored the row replaces
//                    it, every other query finds it in its slot of the score matrix.  After it sc[q][d] is what pKF2->m*Score holds
//                    while the reference runs query q, and kf_score[d] what the last query leaves.
//   k_place_select   a workgroup per query: acc and holder of every scored row (<= 10 neighbours, float32 additions in cov order), then
//                    the selection.  De-duplication is an integer atomicMin of list positions per holder, the output an ordered
//                    compaction by wave 0's ballots; the N-best sort is a rank by (acc descending, list position), which is what a stable
//                    sort gives.
// The ranks count in tiles of keys held in LDS; lists of any length take the same path.  No scratch memory, no inline assembly, no float
// atomics; nothing depends on scheduling.
// The pair pass is this file; everything after it -- and the wave that intersects one pair -- is shared with liborbx_placeindex.so and
// lies in orbx_place_kernels.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <string>

#include "../side/orbx_bowvec_device.h"
#include "../side/orbx_handle.h"
#include "../../../include/orbx_place.h"
#include "orbx_place_kernels.h"

namespace {

using orbx::side::Side;
using orbx::side::side_row;

constexpr int kPlaceLds = 4096;           // entries of one query staged in LDS: 16 KiB of ids, 32 KiB of values (ORBX_PLACE_LDS lowers it)
constexpr int kWaves = 8;                 // waves of a k_place_pairs workgroup
constexpr int kThreads = kWaves * 64;
constexpr int kTile = 32;                 // database vectors of a k_place_pairs workgroup
static_assert(kTile % kWaves == 0, "every wave the same number of pairs");

__global__ __launch_bounds__(kThreads) void k_place_pairs(Side q, Side db, int ndb, int tiles, int lds_limit, Work w) {
  __shared__ __align__(16) uint32_t s_id[kPlaceLds + 4];
  __shared__ __align__(16) double s_v[kPlaceLds + 2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qidx = blockIdx.x / tiles, tile = blockIdx.x - qidx * tiles;
  size_t qs;
  int qn;
  side_row(q, qidx, &qs, &qn);
  const uint32_t* const gi = q.ids + qs;
  const double* const gv = q.vals + qs;
  const bool staged = qn <= lds_limit;    // uniform over the workgroup
  int mi = 0, mv = 0;
  if (staged) {
    orbx::side::stage_row(gi, gv, qn, s_id, s_v, tid, kThreads, &mi, &mv);
    __syncthreads();
  }
  for (int k = wave; k < kTile; k += kWaves) {
    const int d = tile * kTile + k;
    if (d >= ndb) break;                  // uniform over the wave
    size_t ds;
    int dn, words;
    uint32_t first;
    double sum;
    side_row(db, d, &ds, &dn);
    if (staged) place_pair_wave(s_id + mi, s_v + mv, qn, db.ids + ds, db.vals + ds, dn, lane, &words, &first, &sum);
    else place_pair_wave(gi, gv, qn, db.ids + ds, db.vals + ds, dn, lane, &words, &first, &sum);
    if (lane == 0) {
      const size_t o = (size_t)qidx * ndb + d;
      w.words[o] = words;
      w.first[o] = first;
      w.sc[o] = (float)(-sum / 2.0);      // float si = mpVoc->score(...)
    }
  }
}


}  // namespace

struct orbx_place : orbx::side::Handle {
  int lds_limit = kPlaceLds;              // ORBX_PLACE_LDS at create
};

namespace {

using namespace orbx::side;

// the five launches on `st`; every pointer a device pointer
int run(orbx_place* p, hipStream_t st, int kind, int n_candidates, const orbx_place_db* db, const orbx_place_queries* q, int ccap, int32_t* d_cand,
        int32_t* d_ncand, int32_t* d_merge, int32_t* d_nmerge, int32_t* d_stats) {
  const int nq = q->count, ndb = db->count;
  Work w;
  int rc = make_work(p, nq, ndb, &w);
  if (rc != ORBX_OK) return rc;
  if ((rc = wait_previous(p, st)) != ORBX_OK) return rc;
  ORBX_SIDE_HIP(p, hipMemsetAsync(w.db_bad, 0, 4, st));
  const int per_row = (ndb + 255) / 256, tiles = (ndb + kTile - 1) / kTile;
  hipLaunchKernelGGL(k_place_check, dim3(per_row), dim3(256), 0, st, db->d_n, db->stride, db->d_kf_cov, ndb, w.db_bad);
  const Side sq = {q->d_ids, q->d_vals, q->d_n, nullptr, q->stride}, sdb = {db->d_ids, db->d_vals, db->d_n, nullptr, db->stride};
  hipLaunchKernelGGL(k_place_pairs, dim3((unsigned)nq * (unsigned)tiles), dim3(kThreads), 0, st, sq, sdb, ndb, tiles, p->lds_limit, w);
  hipLaunchKernelGGL(k_place_members, dim3(nq), dim3(kSel), 0, st, q->d_n, q->stride, q->d_excl_ptr, q->d_excl_idx, q->n_excl, ndb, w, d_ncand,
                     d_nmerge, d_stats);
  hipLaunchKernelGGL(k_place_scan, dim3(per_row), dim3(256), 0, st, nq, ndb, w, db->d_kf_score);
  hipLaunchKernelGGL(k_place_select, dim3(nq), dim3(kSel), 0, st, kind, n_candidates, ndb, db->d_kf_map, db->d_kf_cov, q->d_q_map, w, ccap, d_cand,
                     d_ncand, d_merge, d_nmerge);
  return ORBX_OK;
}

}  // namespace

extern "C" {

int orbx_place_create(orbx_place** out, int device) {
  return create_handle(out, device, "orbx_place_create", orbx_place_destroy, [](orbx_place* p) {
    p->lds_limit = env_int("ORBX_PLACE_LDS", 0, kPlaceLds, kPlaceLds);
    return (const char*)nullptr;
  });
}

void orbx_place_destroy(orbx_place* p) { destroy_handle(p); }

const char* orbx_place_last_error(const orbx_place* p) { return last_error(p); }

int orbx_place_query_device(orbx_place* p, int kind, int n_candidates, const orbx_place_db* db, const orbx_place_queries* q, int ccap,
                            int32_t* d_cand, int32_t* d_ncand, int32_t* d_merge, int32_t* d_nmerge, int32_t* d_stats, void* stream) {
  if (!p) return ORBX_E_INVALID;
  const std::string who = "orbx_place_query_device: ";
  int rc = check_call(p, who, kind, n_candidates, db, q, ccap, d_cand, d_ncand, d_merge, d_nmerge, d_stats);
  if (rc != ORBX_OK) return rc;
  rc = same_device(p, who.c_str(), {db->d_ids, db->d_vals, db->d_n, db->d_kf_map, db->d_kf_cov, db->d_kf_score, q->d_ids, q->d_vals, q->d_n, q->d_q_map,
                                    q->d_excl_ptr, q->d_excl_idx, d_cand, d_ncand, d_merge, d_nmerge, d_stats}, "the handle");
  if (rc != ORBX_OK) return rc;
  ORBX_SIDE_HIP(p, hipSetDevice(p->device));
  hipStream_t st = stream ? (hipStream_t)stream : p->st;
  if ((rc = run(p, st, kind, n_candidates, db, q, ccap, d_cand, d_ncand, d_merge, d_nmerge, d_stats)) != ORBX_OK) return rc;
  return record_call(p, st);
}

int orbx_place_query(orbx_place* p, int kind, int n_candidates, const orbx_place_db* db, const orbx_place_queries* q, int ccap, int32_t* cand,
                     int32_t* ncand, int32_t* merge, int32_t* nmerge, int32_t* stats) {
  if (!p) return ORBX_E_INVALID;
  const std::string who = "orbx_place_query: ";
  int rc = check_call(p, who, kind, n_candidates, db, q, ccap, cand, ncand, merge, nmerge, stats);
  if (rc != ORBX_OK) return rc;
  if ((rc = check_host_arrays(p, who, db, q)) != ORBX_OK) return rc;
  HostCall c;
  if ((rc = stage_host_call(p, db, q, ccap, cand, ncand, merge, nmerge, stats, &c)) != ORBX_OK) return rc;
  if ((rc = run(p, p->st, kind, n_candidates, &c.db, &c.q, ccap, c.cand, c.ncand, c.merge, c.nmerge, c.stats)) != ORBX_OK) return rc;
  ORBX_SIDE_HIP(p, hipGetLastError());
  return download(p, c.io);
}

}  // extern "C"
