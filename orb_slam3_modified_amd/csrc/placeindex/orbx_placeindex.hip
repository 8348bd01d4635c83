// Place recognition through a device inverted file (include/orbx_placeindex.h): the candidates of orbx_place_query_device, with the
// membership step of KeyFrameDatabase (src/KeyFrameDatabase.cc:617-640, :745-760) -- a walk over the lists of the query's words -- in the
// place of the visit to every (query, database row) pair.  Everything after membership is ../place/orbx_place_kernels.h.
// The sync, a rebuild of the file (CSR by word: ptr[n_words + 1], post_row):
//   k_index_hist     a wave per database row: the snapshot of its count, and an integer atomicAdd on the counter of every id < n_words;
//                    an id >= n_words or a count above the stride sets the file's sync_bad word
//   k_scan_tile / k_scan_add   the exclusive scan over the words, in place: a workgroup per tile (ORBX_PLACEINDEX_SCAN_TILE words), the
//                    tile totals scanned the same way one level up, then added back; the grand total becomes ptr[n_words]
//   k_index_scatter  a wave per row again: post_row[atomicAdd(cursor[id], 1)] = row.  The order inside a list is the cursors'.
// The query:
//   k_place_check, k_index_stale   the dense call's database checks; the current d_n against the snapshot, sync_bad, a count below the
//                    synced count: db_bad
//   (clear)          words = 0, first = UINT32_MAX for Q x D
//   k_index_count    2^g lanes per (query, query entry), striding over the word's list: for every posting of a row that is live NOW an
//                    integer atomicAdd on words[q][row] and an integer atomicMin of the word on first[q][row].  Sums and minima of
//                    integers: the order of the list, and of the lanes, is free.
//   k_index_tail     rows [synced, D): a wave per pair as k_place_pairs, on place_pair_wave: words, first and sc; query 0's workgroups
//                    also hold the tail's ids to n_words
//   k_place_members  unchanged
//   k_index_score    a wave per SCORED pair (the grid is sized for the worst case; a workgroup beyond its query's scored count leaves at
//                    once): place_pair_wave on the two rows, the ordered L1 sum narrowed to float -- the one place a float is added, in
//                    ascending word id as in the dense call
//   k_place_scan, k_place_select   unchanged
// 1-D grids whose workgroup b works on item (b % 8) * chunk + b / 8: the workgroups of one query share an XCD and its L2.  No scratch
// memory, no inline assembly, no float atomics; nothing depends on scheduling.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <string>
#include <vector>

#include "../side/orbx_bowvec_device.h"
#include "../side/orbx_handle.h"
#include "../../../include/orbx_placeindex.h"
#include "../place/orbx_place_kernels.h"

namespace {

using orbx::side::Side;
using orbx::side::side_row;

constexpr int kPlaceLds = 4096;           // entries of one query staged in LDS by the pair passes (ORBX_PLACE_LDS lowers it)
constexpr int kWaves = 8;                 // waves of a pair-pass workgroup
constexpr int kThreads = kWaves * 64;
constexpr int kTile = 32;                 // pairs of a pair-pass workgroup
constexpr int kBlock = 256;               // threads of every other workgroup
constexpr int kScanTile = 2048;           // words of one scan workgroup (ORBX_PLACEINDEX_SCAN_TILE lowers it)
constexpr int kGroupShift = 4;            // 2^4 lanes per query entry in k_index_count (ORBX_PLACEINDEX_GROUP)
static_assert(kTile % kWaves == 0, "every wave the same number of pairs");

// XCD-aware order of a 1-D grid of xcd_grid(nitems) workgroups: the item of this workgroup, which may lie beyond nitems
__device__ __forceinline__ int xcd_item(int nitems) { return (int)(blockIdx.x & 7) * ((nitems + 7) >> 3) + (int)(blockIdx.x >> 3); }
inline unsigned xcd_grid(int nitems) { return (unsigned)(8 * ((nitems + 7) / 8)); }

// ---- sync ----
__global__ __launch_bounds__(kBlock) void k_index_hist(const uint32_t* __restrict__ ids, const int32_t* __restrict__ db_n, int stride, int count,
                                                       int n_words, int32_t* __restrict__ snap, int32_t* hist, int32_t* sync_bad) {
  const int d = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (d >= count) return;                 // uniform over the wave
  const int n = db_n[d];
  if (lane == 0) snap[d] = n;
  bool bad = n > stride;
  const int dn = min(max(n, 0), stride);
  const uint32_t* const row = ids + (size_t)d * stride;
  for (int j = lane; j < dn; j += 64) {
    const uint32_t id = row[j];
    if (id < (uint32_t)n_words) atomicAdd(&hist[id], 1);
    else bad = true;
  }
  if (bad) atomicOr(sync_bad, 1);
}

__global__ __launch_bounds__(kBlock) void k_index_scatter(const uint32_t* __restrict__ ids, const int32_t* __restrict__ db_n, int stride, int count,
                                                          int n_words, int32_t* cursor, int32_t* __restrict__ post_row, int room) {
  const int d = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (d >= count) return;
  const int dn = min(max(db_n[d], 0), stride);
  const uint32_t* const row = ids + (size_t)d * stride;
  for (int j = lane; j < dn; j += 64) {
    const uint32_t id = row[j];
    if (id >= (uint32_t)n_words) continue;
    const int pos = atomicAdd(&cursor[id], 1);
    if (pos >= 0 && pos < room) post_row[pos] = d;      // the histogram counted the same entries: always so unless the arrays changed in between
  }
}

// the exclusive scan of one tile of `tile` words, in place, by one workgroup in chunks of kBlock with a running carry; sums[b] = the tile's total
__global__ __launch_bounds__(kBlock) void k_scan_tile(int32_t* data, int32_t* __restrict__ sums, int n, int tile) {
  __shared__ int s_w[kBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t0 = blockIdx.x * tile, t1 = min(n, t0 + tile);
  int carry = 0;
  for (int base = t0; base < t1; base += kBlock) {    // uniform over the workgroup
    const int i = base + tid;
    const int v = i < t1 ? data[i] : 0;
    int incl = v;
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(incl, o);
      if (lane >= o) incl += t;
    }
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    int off = 0, total = 0;
    for (int k = 0; k < kBlock / 64; k++) { if (k < wave) off += s_w[k]; total += s_w[k]; }
    if (i < t1) data[i] = carry + off + incl - v;
    carry += total;
    __syncthreads();
  }
  if (tid == 0) sums[blockIdx.x] = carry;
}

__global__ __launch_bounds__(kBlock) void k_scan_add(int32_t* __restrict__ data, const int32_t* __restrict__ sums, int n, int tile) {
  const int t0 = blockIdx.x * tile, t1 = min(n, t0 + tile);
  const int add = sums[blockIdx.x];
  for (int i = t0 + threadIdx.x; i < t1; i += kBlock) data[i] += add;
}

// ---- query ----
__global__ void k_index_stale(const int32_t* __restrict__ db_n, const int32_t* __restrict__ snap, int rows, const int32_t* __restrict__ sync_bad,
                              int force_bad, int32_t* db_bad) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  bool bad = d == 0 && (force_bad || *sync_bad != 0);
  if (d < rows) {
    const int c = db_n[d];
    bad |= c >= 0 && c != snap[d];        // erased since the sync (c < 0) is the one change the file allows
  }
  if (bad) atomicOr(db_bad, 1);
}

__global__ __launch_bounds__(kBlock) void k_index_count(const uint32_t* __restrict__ q_ids, const int32_t* __restrict__ q_n, int q_stride, int chunks,
                                                        int shift, const int32_t* __restrict__ ptr, const int32_t* __restrict__ post_row, int n_words,
                                                        const int32_t* __restrict__ db_n, int ndb, Work w, int nitems) {
  const int item = xcd_item(nitems);
  if (item >= nitems || *w.db_bad != 0) return;          // a stale file may hold rows beyond ndb: nothing is read through it
  const int q = item / chunks, chunk = item - q * chunks;
  const int qn = min(max(q_n[q], 0), q_stride);
  const int e = chunk * (kBlock >> shift) + ((int)threadIdx.x >> shift), sub = (int)threadIdx.x & ((1 << shift) - 1);
  if (e >= qn) return;
  const uint32_t word = q_ids[(size_t)q * q_stride + e];
  if (word >= (uint32_t)n_words) return;                 // no postings
  const size_t row = (size_t)q * ndb;
  const int k1 = ptr[word + 1];
  for (int k = ptr[word] + sub; k < k1; k += 1 << shift) {
    const int d = post_row[k];
    if (d < 0 || d >= ndb || db_n[d] < 0) continue;      // erased now
    atomicAdd(&w.words[row + d], 1);
    atomicMin(&w.first[row + d], word);
  }
}

// The two pair passes: the pairs of one query by one workgroup, a wave each, the query staged in LDS as in k_place_pairs.  In the tail
// pass pair i is row d0 + i and the wave stores all three results; in the score pass pair i is the query's i-th scored row, of which the
// rows below d0 still lack their score.
__global__ __launch_bounds__(kThreads) void k_index_tail(Side q, Side db, int nq, int ndb, int d0, int tiles, int lds_limit, int n_words, Work w) {
  __shared__ __align__(16) uint32_t s_id[kPlaceLds + 4];
  __shared__ __align__(16) double s_v[kPlaceLds + 2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int item = xcd_item(nq * tiles);
  if (item >= nq * tiles) return;
  const int qidx = item / tiles, tile = item - qidx * tiles;
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
    const int d = d0 + tile * kTile + k;
    if (d >= ndb) break;                  // uniform over the wave
    size_t ds;
    int dn, words;
    uint32_t first;
    double sum;
    side_row(db, d, &ds, &dn);
    if (qidx == 0) {                      // once a call: the tail's ids, which no sync has seen yet
      bool bad = false;
      for (int j = lane; j < dn; j += 64) bad |= db.ids[ds + j] >= (uint32_t)n_words;
      if (bad) atomicOr(w.db_bad, 1);
    }
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

__global__ __launch_bounds__(kThreads) void k_index_score(Side q, Side db, int nq, int ndb, int d0, int tiles, int lds_limit, Work w) {
  __shared__ __align__(16) uint32_t s_id[kPlaceLds + 4];
  __shared__ __align__(16) double s_v[kPlaceLds + 2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int item = xcd_item(nq * tiles);
  if (item >= nq * tiles) return;
  const int qidx = item / tiles, tile = item - qidx * tiles;
  if (w.qinfo[2 * qidx] != 0) return;     // malformed: scores nothing
  const int n = w.qinfo[2 * qidx + 1];    // the query's scored rows: w.rows[0 .. n)
  if (tile * kTile >= n) return;          // uniform: the grid is sized for n = ndb
  size_t qs;
  int qn;
  side_row(q, qidx, &qs, &qn);
  const uint32_t* const gi = q.ids + qs;
  const double* const gv = q.vals + qs;
  const bool staged = qn <= lds_limit;
  int mi = 0, mv = 0;
  if (staged) {
    orbx::side::stage_row(gi, gv, qn, s_id, s_v, tid, kThreads, &mi, &mv);
    __syncthreads();
  }
  for (int k = wave; k < kTile; k += kWaves) {
    const int i = tile * kTile + k;
    if (i >= n) break;                    // uniform over the wave
    const int d = w.rows[(size_t)qidx * ndb + i];
    if (d >= d0) continue;                // a tail row: k_index_tail left its score
    size_t ds;
    int dn, words;
    uint32_t first;
    double sum;
    side_row(db, d, &ds, &dn);
    if (staged) place_pair_wave(s_id + mi, s_v + mv, qn, db.ids + ds, db.vals + ds, dn, lane, &words, &first, &sum);
    else place_pair_wave(gi, gv, qn, db.ids + ds, db.vals + ds, dn, lane, &words, &first, &sum);
    if (lane == 0) w.sc[(size_t)qidx * ndb + d] = (float)(-sum / 2.0);
  }
}

}  // namespace

struct orbx_placeindex : orbx::side::Handle {
  int n_words = 0;
  int lds_limit = kPlaceLds;              // ORBX_PLACE_LDS at create
  int scan_tile = kScanTile;              // ORBX_PLACEINDEX_SCAN_TILE at create
  int group_shift = kGroupShift;          // ORBX_PLACEINDEX_GROUP at create, as a shift
  int synced = 0;                         // rows of the database the file indexes; 0: no file
  orbx::side::Block file;                 // ptr [n_words + 1], cursor [n_words], the scan's tile totals, sync_bad [1]
  orbx::side::Block post;                 // post_row, room for count * stride postings
  orbx::side::Block snap;                 // d_n[0 .. synced) at the sync
  int32_t *ptr = nullptr, *cursor = nullptr, *sums = nullptr, *sync_bad = nullptr;
  std::vector<size_t> level;              // where each scan level's tile totals begin in `sums`
};

namespace {

using namespace orbx::side;

// the file's fixed arrays; what failed, or nullptr
const char* make_file(orbx_placeindex* p) {
  size_t totals = 0;
  for (int n = p->n_words;;) {
    const int nb = (n + p->scan_tile - 1) / p->scan_tile;
    p->level.push_back(totals);
    totals += (size_t)nb;
    if (nb == 1) break;
    n = nb;
  }
  Layout lay;
  const size_t o_ptr = lay.add(((size_t)p->n_words + 1) * 4), o_cur = lay.add((size_t)p->n_words * 4), o_sums = lay.add(totals * 4), o_bad = lay.add(4);
  if (hipMalloc((void**)&p->file.p, lay.size) != hipSuccess) { (void)hipGetLastError(); return "the inverted file's arrays could not be allocated"; }
  p->file.bytes = lay.size;
  p->ptr = (int32_t*)(p->file.p + o_ptr); p->cursor = (int32_t*)(p->file.p + o_cur);
  p->sums = (int32_t*)(p->file.p + o_sums); p->sync_bad = (int32_t*)(p->file.p + o_bad);
  return nullptr;
}

// exclusive scan of data[0 .. n) in place; the level's tile totals are scanned the same way.  The grand total ends in sums[level.back()]
void scan_level(orbx_placeindex* p, hipStream_t st, int32_t* data, int n, size_t lv) {
  const int nb = (n + p->scan_tile - 1) / p->scan_tile;
  int32_t* const totals = p->sums + p->level[lv];
  hipLaunchKernelGGL(k_scan_tile, dim3(nb), dim3(kBlock), 0, st, data, totals, n, p->scan_tile);
  if (nb == 1) return;
  scan_level(p, st, totals, nb, lv + 1);
  hipLaunchKernelGGL(k_scan_add, dim3(nb), dim3(kBlock), 0, st, data, (const int32_t*)totals, n, p->scan_tile);
}

// the rebuild on `st`; d_ids and d_n device pointers
int sync_run(orbx_placeindex* p, hipStream_t st, const orbx_place_db* db) {
  p->synced = 0;                          // a rebuild that fails leaves no file
  const int count = db->count, room = count * db->stride;
  int rc = grow(p, &p->post, (size_t)room * 4);
  if (rc != ORBX_OK || (rc = grow(p, &p->snap, (size_t)count * 4)) != ORBX_OK) return rc;
  if ((rc = wait_previous(p, st)) != ORBX_OK) return rc;
  ORBX_SIDE_HIP(p, hipMemsetAsync(p->ptr, 0, ((size_t)p->n_words + 1) * 4, st));
  ORBX_SIDE_HIP(p, hipMemsetAsync(p->sync_bad, 0, 4, st));
  const int grid = (count + kBlock / 64 - 1) / (kBlock / 64);
  hipLaunchKernelGGL(k_index_hist, dim3(grid), dim3(kBlock), 0, st, db->d_ids, db->d_n, db->stride, count, p->n_words, (int32_t*)p->snap.p, p->ptr,
                     p->sync_bad);
  scan_level(p, st, p->ptr, p->n_words, 0);
  ORBX_SIDE_HIP(p, hipMemcpyAsync(p->ptr + p->n_words, p->sums + p->level.back(), 4, hipMemcpyDeviceToDevice, st));
  ORBX_SIDE_HIP(p, hipMemcpyAsync(p->cursor, p->ptr, (size_t)p->n_words * 4, hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(k_index_scatter, dim3(grid), dim3(kBlock), 0, st, db->d_ids, db->d_n, db->stride, count, p->n_words, p->cursor,
                     (int32_t*)p->post.p, room);
  p->synced = count;
  return ORBX_OK;
}

// the query's launches on `st`; every pointer a device pointer
int run(orbx_placeindex* p, hipStream_t st, int kind, int n_candidates, const orbx_place_db* db, const orbx_place_queries* q, int ccap,
        int32_t* d_cand, int32_t* d_ncand, int32_t* d_merge, int32_t* d_nmerge, int32_t* d_stats) {
  const int nq = q->count, ndb = db->count;
  Work w;
  int rc = make_work(p, nq, ndb, &w);
  if (rc != ORBX_OK) return rc;
  if ((rc = wait_previous(p, st)) != ORBX_OK) return rc;
  ORBX_SIDE_HIP(p, hipMemsetAsync(w.db_bad, 0, 4, st));
  const int per_row = (ndb + 255) / 256;
  hipLaunchKernelGGL(k_place_check, dim3(per_row), dim3(256), 0, st, db->d_n, db->stride, db->d_kf_cov, ndb, w.db_bad);
  const bool shrunk = ndb < p->synced;    // the database lost rows the file holds: every query is malformed
  const int d0 = std::min(p->synced, ndb);
  const Side sq = {q->d_ids, q->d_vals, q->d_n, nullptr, q->stride}, sdb = {db->d_ids, db->d_vals, db->d_n, nullptr, db->stride};
  if (p->synced > 0) {
    hipLaunchKernelGGL(k_index_stale, dim3((d0 + 255) / 256), dim3(256), 0, st, db->d_n, (const int32_t*)p->snap.p, d0, (const int32_t*)p->sync_bad,
                       shrunk ? 1 : 0, w.db_bad);
    if (!shrunk) {
      const size_t cells = (size_t)nq * ndb * 4;
      ORBX_SIDE_HIP(p, hipMemsetAsync(w.words, 0, cells, st));
      ORBX_SIDE_HIP(p, hipMemsetAsync(w.first, 0xff, cells, st));
      const int per = kBlock >> p->group_shift, chunks = (q->stride + per - 1) / per;
      if ((long long)nq * chunks > (long long)INT_MAX - 8) return fail(p, ORBX_E_INVALID, "orbx_placeindex: Q * query stride exceeds what one grid holds");
      hipLaunchKernelGGL(k_index_count, dim3(xcd_grid(nq * chunks)), dim3(kBlock), 0, st, q->d_ids, q->d_n, q->stride, chunks, p->group_shift,
                         (const int32_t*)p->ptr, (const int32_t*)p->post.p, p->n_words, db->d_n, ndb, w, nq * chunks);
    }
  }
  if (ndb > d0) {
    const int tiles = (ndb - d0 + kTile - 1) / kTile;
    hipLaunchKernelGGL(k_index_tail, dim3(xcd_grid(nq * tiles)), dim3(kThreads), 0, st, sq, sdb, nq, ndb, d0, tiles, p->lds_limit, p->n_words, w);
  }
  hipLaunchKernelGGL(k_place_members, dim3(nq), dim3(kSel), 0, st, q->d_n, q->stride, q->d_excl_ptr, q->d_excl_idx, q->n_excl, ndb, w, d_ncand,
                     d_nmerge, d_stats);
  if (d0 > 0) {
    const int tiles = (ndb + kTile - 1) / kTile;
    hipLaunchKernelGGL(k_index_score, dim3(xcd_grid(nq * tiles)), dim3(kThreads), 0, st, sq, sdb, nq, ndb, d0, tiles, p->lds_limit, w);
  }
  hipLaunchKernelGGL(k_place_scan, dim3(per_row), dim3(256), 0, st, nq, ndb, w, db->d_kf_score);
  hipLaunchKernelGGL(k_place_select, dim3(nq), dim3(kSel), 0, st, kind, n_candidates, ndb, db->d_kf_map, db->d_kf_cov, q->d_q_map, w, ccap, d_cand,
                     d_ncand, d_merge, d_nmerge);
  return ORBX_OK;
}

int check_sync(orbx_placeindex* p, const std::string& who, const orbx_place_db* db) {
  if (!db) return fail(p, ORBX_E_INVALID, who + "null argument");
  if (!db->d_ids || !db->d_n) return fail(p, ORBX_E_INVALID, who + "null buffer");
  if (db->count < 1 || db->stride < 1) return fail(p, ORBX_E_INVALID, who + "count and stride must be at least 1");
  if ((long long)db->count * (long long)db->stride > (long long)INT_MAX) return fail(p, ORBX_E_INVALID, who + "count * stride exceeds INT_MAX");
  return ORBX_OK;
}

}  // namespace

extern "C" {

int orbx_placeindex_create(orbx_placeindex** out, int device, int n_words) {
  const char* const who = "orbx_placeindex_create";
  if (out) *out = nullptr;
  if (out && device >= 0 && (n_words < 1 || n_words > ORBX_PLACEINDEX_MAX_WORDS))
    return create_fail(ORBX_E_INVALID, who, "n_words must lie in [1, ORBX_PLACEINDEX_MAX_WORDS]");
  return create_handle(out, device, who, orbx_placeindex_destroy, [n_words](orbx_placeindex* p) {
    p->n_words = n_words;
    p->lds_limit = env_int("ORBX_PLACE_LDS", 0, kPlaceLds, kPlaceLds);
    p->scan_tile = env_int("ORBX_PLACEINDEX_SCAN_TILE", 2, kScanTile, kScanTile);
    const int group = env_int("ORBX_PLACEINDEX_GROUP", 1, 64, 1 << kGroupShift);
    for (p->group_shift = 0; (2 << p->group_shift) <= group; p->group_shift++) {}
    return make_file(p);
  });
}

void orbx_placeindex_destroy(orbx_placeindex* p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  if (p->pending && p->ev_done) (void)hipEventSynchronize(p->ev_done);
  if (p->st) (void)hipStreamSynchronize(p->st);
  for (Block* b : {&p->file, &p->post, &p->snap})
    if (b->p) (void)hipFree(b->p);
  destroy_handle(p);
}

const char* orbx_placeindex_last_error(const orbx_placeindex* p) { return last_error(p); }

int orbx_placeindex_sync_device(orbx_placeindex* p, const orbx_place_db* db, void* stream) {
  if (!p) return ORBX_E_INVALID;
  const std::string who = "orbx_placeindex_sync_device: ";
  int rc = check_sync(p, who, db);
  if (rc != ORBX_OK) return rc;
  if ((rc = same_device(p, who.c_str(), {db->d_ids, db->d_n}, "the handle")) != ORBX_OK) return rc;
  ORBX_SIDE_HIP(p, hipSetDevice(p->device));
  hipStream_t st = stream ? (hipStream_t)stream : p->st;
  if ((rc = sync_run(p, st, db)) != ORBX_OK) return rc;
  return record_call(p, st);
}

int orbx_placeindex_query_device(orbx_placeindex* p, int kind, int n_candidates, const orbx_place_db* db, const orbx_place_queries* q, int ccap,
                                 int32_t* d_cand, int32_t* d_ncand, int32_t* d_merge, int32_t* d_nmerge, int32_t* d_stats, void* stream) {
  if (!p) return ORBX_E_INVALID;
  const std::string who = "orbx_placeindex_query_device: ";
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

int orbx_placeindex_query(orbx_placeindex* p, int kind, int n_candidates, const orbx_place_db* db, const orbx_place_queries* q, int ccap,
                          int32_t* cand, int32_t* ncand, int32_t* merge, int32_t* nmerge, int32_t* stats) {
  if (!p) return ORBX_E_INVALID;
  const std::string who = "orbx_placeindex_query: ";
  int rc = check_call(p, who, kind, n_candidates, db, q, ccap, cand, ncand, merge, nmerge, stats);
  if (rc != ORBX_OK || (rc = check_sync(p, who, db)) != ORBX_OK || (rc = check_host_arrays(p, who, db, q)) != ORBX_OK) return rc;
  for (int d = 0; d < db->count; d++)
    for (int j = 0; j < db->d_n[d]; j++)
      if (db->d_ids[(size_t)d * db->stride + j] >= (uint32_t)p->n_words)
        return fail(p, ORBX_E_INVALID, who + "database row " + std::to_string(d) + ": word id outside [0, n_words)");
  HostCall c;
  if ((rc = stage_host_call(p, db, q, ccap, cand, ncand, merge, nmerge, stats, &c)) != ORBX_OK) return rc;
  if ((rc = sync_run(p, p->st, &c.db)) != ORBX_OK) return rc;
  rc = run(p, p->st, kind, n_candidates, &c.db, &c.q, ccap, c.cand, c.ncand, c.merge, c.nmerge, c.stats);
  p->synced = 0;                          // the file indexed the upload, not an array of the caller's
  if (rc != ORBX_OK) return rc;
  ORBX_SIDE_HIP(p, hipGetLastError());
  return download(p, c.io);
}

}  // extern "C"
