// What liborbx_place.so (orbx_place.hip) and liborbx_placeindex.so (../placeindex/orbx_placeindex.hip) share: the call's intermediate
// arrays, the wave that intersects one (query, database row) pair, the per-query membership and selection workgroups, the column scan
// between them, and the host side's argument checks and staging.  One query path after membership: the two libraries differ only in how
// `words`, `first` and the scored pairs' `sc` come about.  Below csrc/, outside kernels_hash().
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <string>

#include "../side/orbx_bowvec_device.h"
#include "../side/orbx_handle.h"
#include "../../../include/orbx_place.h"

namespace {

constexpr int kSel = 256;                 // threads of the per-query workgroups
constexpr int kSelWaves = kSel / 64;
constexpr int kRankTile = 1024;           // keys of one ranking tile in LDS
constexpr int kCov = ORBX_PLACE_COV;

// the call's intermediate arrays, [nq][ndb] each unless noted
struct Work {
  int32_t* words;    // common words of the pair
  uint32_t* first;   // its lowest common word
  float* sc;         // its score; after k_place_scan: the row's score field as query q finds it
  int32_t* state;    // 0 not in the query, 1 in the query, 2 scored
  int32_t* rows;     // the scored rows, ascending
  int32_t* lst;      // the scored rows in list order
  float* acc;        // per list position
  int32_t* holder;   // per list position
  int32_t* seen;     // per row: the first position that holds it
  int32_t* order;    // N-best: list positions by (acc descending, position)
  int32_t* qinfo;    // [nq][2] = {malformed, scored rows}
  int32_t* db_bad;   // [1]
};

__global__ void k_place_check(const int32_t* __restrict__ db_n, int stride, const int32_t* __restrict__ cov, int ndb, int32_t* db_bad) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= ndb) return;
  bool bad = db_n[d] > stride;
  for (int k = 0; k < kCov; k++) bad |= cov[(size_t)d * kCov + k] >= ndb;
  if (bad) atomicOr(db_bad, 1);
}

// One pair by one wave: the same values in every lane.  qi / qv: the query (LDS or global), di / dv: the database vector (global).
__device__ __forceinline__ void place_pair_wave(const uint32_t* qi, const double* qv, int qn, const uint32_t* di, const double* dv, int dn,
                                                int lane, int* words, uint32_t* first, double* sum) {
  double score = 0;
  int cnt = 0;
  uint32_t fw = 0;
  for (int base = 0; base < dn; base += 64) {
    const int j = base + lane;
    bool hit = false;
    double t = 0;
    uint32_t id = 0;
    if (j < dn) {
      id = di[j];
      const int lo = orbx::side::first_not_below(qi, qn, id);
      if (lo < qn && qi[lo] == id) {
        const double vi = qv[lo], wi = dv[j];
        t = __dsub_rn(__dsub_rn(fabs(__dsub_rn(vi, wi)), fabs(vi)), fabs(wi));
        hit = true;
      }
    }
    unsigned long long m = __ballot(hit);
    if (m) {                              // uniform over the wave: ascending lane = ascending word id
      if (cnt == 0) fw = (uint32_t)__builtin_amdgcn_readlane((int)id, __builtin_ctzll(m));
      cnt += __popcll(m);
    }
    const int thi = __double2hiint(t), tlo = __double2loint(t);
    while (m) {
      const int l = __builtin_ctzll(m);
      m &= m - 1;
      score = __dadd_rn(score, __hiloint2double(__builtin_amdgcn_readlane(thi, l), __builtin_amdgcn_readlane(tlo, l)));
    }
  }
  *words = cnt; *first = fw; *sum = score;
}

// ---- per-query workgroups of kSel threads ----
__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (1ull << lane) - 1ull; }

// the same value in every thread; s_red: kSelWaves words.  The barriers make the helper safe to call again at once
__device__ __forceinline__ int block_max(int v, int* s_red, int tid) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  if ((tid & 63) == 0) s_red[tid >> 6] = v;
  __syncthreads();
  int r = s_red[0];
  for (int k = 1; k < kSelWaves; k++) r = max(r, s_red[k]);
  __syncthreads();
  return r;
}
__device__ __forceinline__ int block_sum(int v, int* s_red, int tid) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((tid & 63) == 0) s_red[tid >> 6] = v;
  __syncthreads();
  int r = s_red[0];
  for (int k = 1; k < kSelWaves; k++) r += s_red[k];
  __syncthreads();
  return r;
}

// position i's rank among n keys: the number of positions j whose key comes first, `before(kj, j, ki, i)`.  key(j) reads position j's
// key; the tiles of keys go through s_key.  Called by the whole workgroup with uniform n and ig; i = ig + tid may lie beyond n.
template <class Key, class Before>
__device__ __forceinline__ int rank_of(int n, int i, uint32_t ki, uint32_t* s_key, int tid, Key key, Before before) {
  int rank = 0;
  for (int t0 = 0; t0 < n; t0 += kRankTile) {
    const int m = min(kRankTile, n - t0);
    __syncthreads();                      // the readers of the tile before
    for (int j = tid; j < m; j += kSel) s_key[j] = key(t0 + j);
    __syncthreads();
    if (i < n)
      for (int j = 0; j < m; j++) rank += before(s_key[j], t0 + j, ki, i) ? 1 : 0;
  }
  return rank;
}

__device__ __forceinline__ bool excluded(const int32_t* ex, int n, int d) {
  int lo = 0, len = n;
  while (len > 0) {
    const int half = len >> 1;
    if (ex[lo + half] < d) { lo += half + 1; len -= half + 1; } else len = half;
  }
  return lo < n && ex[lo] == d;
}

__global__ __launch_bounds__(kSel) void k_place_members(const int32_t* __restrict__ q_n, int q_stride, const int32_t* __restrict__ excl_ptr,
                                                        const int32_t* __restrict__ excl_idx, int n_excl, int ndb, Work w,
                                                        int32_t* __restrict__ ncand, int32_t* __restrict__ nmerge,
                                                        int32_t* __restrict__ stats) {
  __shared__ int s_red[kSelWaves];
  __shared__ uint32_t s_key[kRankTile];
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t row = (size_t)q * ndb;
  // the checks: nothing below addresses memory with a value that has not passed them
  int bad = (*w.db_bad != 0 || q_n[q] > q_stride) ? 1 : 0;
  int e0 = 0, e1 = 0;
  if (excl_ptr) {
    e0 = excl_ptr[q]; e1 = excl_ptr[q + 1];
    if (e0 < 0 || e1 < e0 || e1 > n_excl) { bad = 1; e0 = e1 = 0; }
  }
  for (int e = e0 + tid; e < e1; e += kSel) {
    const int v = excl_idx[e];
    if (v < 0 || v >= ndb || (e > e0 && excl_idx[e - 1] >= v)) bad = 1;
  }
  bad = __syncthreads_or(bad);
  if (bad) {                              // uniform: the query scores nothing and keeps its output rows
    for (int d = tid; d < ndb; d += kSel) w.state[row + d] = 0;
    if (tid == 0) {
      w.qinfo[2 * q] = 1; w.qinfo[2 * q + 1] = 0;
      ncand[q] = -1;
      if (nmerge) nmerge[q] = -1;
    }
    return;
  }
  const int32_t* const ex = excl_idx + e0;
  int mx = 0, nmem = 0;
  for (int d = tid; d < ndb; d += kSel) {
    const int wd = w.words[row + d];
    const bool mem = wd > 0 && !excluded(ex, e1 - e0, d);
    w.state[row + d] = mem ? 1 : 0;
    if (mem) { mx = max(mx, wd); nmem++; }
  }
  const int max_common = block_max(mx, s_red, tid);
  nmem = block_sum(nmem, s_red, tid);
  const int min_common = (int)((float)max_common * 0.8f);
  // the scored rows, ascending: each thread reads back its own state word
  int n = 0;
  for (int base = 0; base < ndb; base += kSel) {
    const int d = base + tid;
    const bool scored = d < ndb && w.state[row + d] == 1 && w.words[row + d] > min_common;
    const unsigned long long m = __ballot(scored);
    if (lane == 0) s_red[wave] = __popcll(m);
    __syncthreads();
    int off = n, total = 0;
    for (int k = 0; k < kSelWaves; k++) { if (k < wave) off += s_red[k]; total += s_red[k]; }
    if (scored) {
      w.rows[row + off + __popcll(m & lanes_below(lane))] = d;
      w.state[row + d] = 2;
    }
    n += total;
    __syncthreads();
  }
  // list order: ascending (lowest common word, row); rows[] ascends, so the position breaks the tie
  const int32_t* const rows = w.rows + row;
  const uint32_t* const first = w.first + row;
  for (int ig = 0; ig < n; ig += kSel) {
    const int i = ig + tid;
    const uint32_t ki = i < n ? first[rows[i]] : 0;
    const int rank = rank_of(n, i, ki, s_key, tid, [&](int j) { return first[rows[j]]; },
                             [](uint32_t kj, int j, uint32_t k, int p) { return kj < k || (kj == k && j < p); });
    if (i < n) w.lst[row + rank] = rows[i];
  }
  if (tid == 0) {
    w.qinfo[2 * q] = 0; w.qinfo[2 * q + 1] = n;
    stats[4 * q] = nmem; stats[4 * q + 1] = n; stats[4 * q + 2] = max_common; stats[4 * q + 3] = min_common;
  }
}

__global__ void k_place_scan(int nq, int ndb, Work w, float* __restrict__ kf_score) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= ndb) return;
  float cur = kf_score[d];
  for (int q = 0; q < nq; q++) {
    const size_t o = (size_t)q * ndb + d;
    if (w.state[o] == 2) cur = w.sc[o];
    else w.sc[o] = cur;
  }
  kf_score[d] = cur;
}

// a float as an unsigned key of the same order (-0 as +0)
__device__ __forceinline__ uint32_t ordered_key(float f) {
  uint32_t u = f == 0.0f ? 0u : __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// `seen` is written by atomicMin, which works in L2: its plain accesses go there too, past the vector L1
__device__ __forceinline__ void seen_reset(int32_t* a) { __hip_atomic_store(a, INT_MAX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int seen_at(int32_t* a) { return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// wave 0: positions [count, ccap) of an output row
__device__ __forceinline__ void fill_rest(int32_t* out, int count, int ccap, int lane) {
  for (int p = max(count, 0) + lane; p < ccap; p += 64) out[p] = -1;
}

__global__ __launch_bounds__(kSel) void k_place_select(int kind, int n_candidates, int ndb, const int32_t* __restrict__ kf_map,
                                                       const int32_t* __restrict__ cov, const int32_t* __restrict__ q_map, Work w, int ccap,
                                                       int32_t* __restrict__ cand, int32_t* __restrict__ ncand, int32_t* __restrict__ merge,
                                                       int32_t* __restrict__ nmerge) {
  __shared__ int s_red[kSelWaves];
  __shared__ uint32_t s_key[kRankTile];
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (w.qinfo[2 * q]) return;             // malformed: uniform
  const int n = w.qinfo[2 * q + 1];
  const size_t row = (size_t)q * ndb;
  const int qmap = q_map[q];
  const float* const sc = w.sc + row;
  const int32_t* const state = w.state + row;
  float* const acc = w.acc + row;
  int32_t* const holder = w.holder + row;
  int32_t* const seen = w.seen + row;
  int32_t* const order = w.order + row;
  int32_t* const cand_row = cand + (size_t)q * ccap;
  float top = 0;                          // bestAccScore, from 0
  for (int i = tid; i < n; i += kSel) {
    const int r = w.lst[row + i];
    float a = sc[r], best = a;
    int h = r;
    for (int k = 0; k < kCov; k++) {
      const int c = cov[(size_t)r * kCov + k];
      if (c < 0 || state[c] == 0) continue;
      const float s2 = sc[c];
      a = a + s2;
      if (s2 > best) { h = c; best = s2; }
    }
    acc[i] = a; holder[i] = h;
    if (a > top) top = a;
  }
  if (kind == ORBX_PLACE_RELOC) {
    const float min_retain = 0.75f * __uint_as_float((uint32_t)block_max((int)__float_as_uint(top), s_red, tid));   // top >= +0: its bits order as ints
    // (block_max's barriers also publish acc and holder)
    for (int i = tid; i < n; i += kSel)
      if (acc[i] > min_retain && kf_map[holder[i]] == qmap) seen_reset(&seen[holder[i]]);
    __syncthreads();
    for (int i = tid; i < n; i += kSel)
      if (acc[i] > min_retain && kf_map[holder[i]] == qmap) atomicMin(&seen[holder[i]], i);
    __syncthreads();
    if (wave != 0) return;
    int count = 0;
    for (int base = 0; base < n; base += 64) {
      const int i = base + lane;
      int h = -1;
      bool ok = false;
      if (i < n) {
        h = holder[i];
        ok = acc[i] > min_retain && kf_map[h] == qmap && seen_at(&seen[h]) == i;
      }
      const unsigned long long m = __ballot(ok);
      const int pos = count + __popcll(m & lanes_below(lane));
      if (ok && pos < ccap) cand_row[pos] = h;
      count += __popcll(m);
    }
    fill_rest(cand_row, count, ccap, lane);
    if (lane == 0) ncand[q] = count;
    return;
  }
  // N-best: positions by (acc descending, position ascending)
  __syncthreads();
  for (int ig = 0; ig < n; ig += kSel) {
    const int i = ig + tid;
    const uint32_t ki = i < n ? ordered_key(acc[i]) : 0;
    const int rank = rank_of(n, i, ki, s_key, tid, [&](int j) { return ordered_key(acc[j]); },
                             [](uint32_t kj, int j, uint32_t k, int p) { return kj > k || (kj == k && j < p); });
    if (i < n) order[rank] = i;
  }
  __syncthreads();
  for (int p = tid; p < n; p += kSel) seen_reset(&seen[holder[order[p]]]);
  __syncthreads();
  for (int p = tid; p < n; p += kSel) atomicMin(&seen[holder[order[p]]], p);
  __syncthreads();
  if (wave != 0) return;
  int32_t* const merge_row = merge + (size_t)q * ccap;
  int nl = 0, nm = 0;
  for (int base = 0; base < n && (nl < n_candidates || nm < n_candidates); base += 64) {
    const int p = base + lane;
    int h = -1;
    bool fresh = false, same = false;
    if (p < n) {
      h = holder[order[p]];
      fresh = seen_at(&seen[h]) == p;              // spAlreadyAddedKF: a holder counts where it is met first, taken or not
      same = kf_map[h] == qmap;
    }
    const unsigned long long ml = __ballot(fresh && same), mm = __ballot(fresh && !same);
    const int pl = nl + __popcll(ml & lanes_below(lane)), pm = nm + __popcll(mm & lanes_below(lane));
    if (fresh && same && pl < n_candidates && pl < ccap) cand_row[pl] = h;
    if (fresh && !same && pm < n_candidates && pm < ccap) merge_row[pm] = h;
    nl += __popcll(ml); nm += __popcll(mm);
  }
  nl = min(nl, n_candidates); nm = min(nm, n_candidates);
  fill_rest(cand_row, nl, ccap, lane);
  fill_rest(merge_row, nm, ccap, lane);
  if (lane == 0) { ncand[q] = nl; nmerge[q] = nm; }
}

// ---- host side ----
// what every form checks first
inline int check_call(orbx::side::Handle* p, const std::string& who, int kind, int n_candidates, const orbx_place_db* db, const orbx_place_queries* q,
                      int ccap, const void* cand, const void* ncand, const void* merge, const void* nmerge, const void* stats) {
  using orbx::side::fail;
  if (kind != ORBX_PLACE_RELOC && kind != ORBX_PLACE_NBEST) return fail(p, ORBX_E_INVALID, who + "kind = " + std::to_string(kind) + " (ORBX_PLACE_RELOC or ORBX_PLACE_NBEST)");
  if (!db || !q || !cand || !ncand || !stats) return fail(p, ORBX_E_INVALID, who + "null argument");
  if (!db->d_ids || !db->d_vals || !db->d_n || !db->d_kf_map || !db->d_kf_cov || !db->d_kf_score || !q->d_ids || !q->d_vals || !q->d_n || !q->d_q_map)
    return fail(p, ORBX_E_INVALID, who + "null buffer");
  if (db->count < 1 || q->count < 1 || db->stride < 1 || q->stride < 1 || ccap < 1) return fail(p, ORBX_E_INVALID, who + "counts, strides and ccap must be at least 1");
  if ((long long)db->count * (long long)q->count > (long long)INT_MAX) return fail(p, ORBX_E_INVALID, who + "Q * D exceeds INT_MAX");
  if ((long long)q->count * (long long)ccap > (long long)INT_MAX) return fail(p, ORBX_E_INVALID, who + "Q * ccap exceeds INT_MAX");
  if (q->n_excl < 0 || (q->d_excl_ptr && q->n_excl > 0 && !q->d_excl_idx)) return fail(p, ORBX_E_INVALID, who + "n_excl < 0, or exclusion rows without their indices");
  if (kind == ORBX_PLACE_RELOC && (q->d_excl_ptr || merge || nmerge)) return fail(p, ORBX_E_INVALID, who + "relocalization takes no exclusions and no merge arrays");
  if (kind == ORBX_PLACE_NBEST && (!merge || !nmerge)) return fail(p, ORBX_E_INVALID, who + "N-best needs the merge arrays");
  if (kind == ORBX_PLACE_NBEST && n_candidates < 1) return fail(p, ORBX_E_INVALID, who + "n_candidates must be at least 1");
  return ORBX_OK;
}

// the call's intermediate arrays in the handle's scratch, which is grown for them
inline int make_work(orbx::side::Handle* p, int nq, int ndb, Work* w) {
  const size_t cells = (size_t)nq * ndb * 4;
  orbx::side::Layout lay;
  size_t o[10];
  for (size_t& x : o) x = lay.add(cells);
  const size_t o_qinfo = lay.add((size_t)nq * 8), o_bad = lay.add(4);
  const int rc = orbx::side::grow(p, &p->scratch, lay.size);
  if (rc != ORBX_OK) return rc;
  uint8_t* const s = p->scratch.p;
  *w = {(int32_t*)(s + o[0]), (uint32_t*)(s + o[1]), (float*)(s + o[2]),   (int32_t*)(s + o[3]), (int32_t*)(s + o[4]),
        (int32_t*)(s + o[5]), (float*)(s + o[6]),    (int32_t*)(s + o[7]), (int32_t*)(s + o[8]), (int32_t*)(s + o[9]),
        (int32_t*)(s + o_qinfo), (int32_t*)(s + o_bad)};
  return ORBX_OK;
}

// A host form sees everything: what the device form marks per query is an error here
inline int check_host_arrays(orbx::side::Handle* p, const std::string& who, const orbx_place_db* db, const orbx_place_queries* q) {
  using orbx::side::fail;
  const int nq = q->count, ndb = db->count;
  for (int d = 0; d < ndb; d++) {
    if (db->d_n[d] > db->stride) return fail(p, ORBX_E_INVALID, who + "database row " + std::to_string(d) + ": count above the stride");
    for (int k = 0; k < kCov; k++)
      if (db->d_kf_cov[(size_t)d * kCov + k] >= ndb) return fail(p, ORBX_E_INVALID, who + "database row " + std::to_string(d) + ": covisibility entry outside [0, D)");
  }
  for (int i = 0; i < nq; i++) {
    if (q->d_n[i] > q->stride) return fail(p, ORBX_E_INVALID, who + "query " + std::to_string(i) + ": count above the stride");
    if (!q->d_excl_ptr) continue;
    const int e0 = q->d_excl_ptr[i], e1 = q->d_excl_ptr[i + 1];
    if (e0 < 0 || e1 < e0 || e1 > q->n_excl) return fail(p, ORBX_E_INVALID, who + "query " + std::to_string(i) + ": exclusion row outside [0, n_excl]");
    for (int e = e0; e < e1; e++)
      if (q->d_excl_idx[e] < 0 || q->d_excl_idx[e] >= ndb || (e > e0 && q->d_excl_idx[e - 1] >= q->d_excl_idx[e]))
        return fail(p, ORBX_E_INVALID, who + "query " + std::to_string(i) + ": exclusion indices must lie in [0, D) and ascend strictly");
  }
  return ORBX_OK;
}

// a host form's arguments and results in the handle's io block: the device forms' arguments once upload() has run
struct HostCall {
  orbx::side::Stager io;
  orbx_place_db db;
  orbx_place_queries q;
  int32_t *cand, *ncand, *merge, *nmerge, *stats;
};
inline int stage_host_call(orbx::side::Handle* p, const orbx_place_db* db, const orbx_place_queries* q, int ccap, int32_t* cand, int32_t* ncand,
                           int32_t* merge, int32_t* nmerge, int32_t* stats, HostCall* c) {
  orbx::side::Stager& io = c->io;
  const int nq = q->count, ndb = db->count;
  const size_t dz = (size_t)ndb * db->stride, qz = (size_t)nq * q->stride;
  const size_t o_dv = io.in(db->d_vals, dz * 8), o_qv = io.in(q->d_vals, qz * 8), o_di = io.in(db->d_ids, dz * 4), o_qi = io.in(q->d_ids, qz * 4);
  const size_t o_dn = io.in(db->d_n, (size_t)ndb * 4), o_qn = io.in(q->d_n, (size_t)nq * 4), o_map = io.in(db->d_kf_map, (size_t)ndb * 4);
  const size_t o_cov = io.in(db->d_kf_cov, (size_t)ndb * kCov * 4), o_qm = io.in(q->d_q_map, (size_t)nq * 4);
  size_t o_ep = 0, o_ei = 0;
  if (q->d_excl_ptr) {
    o_ep = io.in(q->d_excl_ptr, ((size_t)nq + 1) * 4);
    if (q->n_excl) o_ei = io.in(q->d_excl_idx, (size_t)q->n_excl * 4);
  }
  const size_t o_sc = io.out(db->d_kf_score, (size_t)ndb * 4, true), o_c = io.out(cand, (size_t)nq * ccap * 4), o_nc = io.out(ncand, (size_t)nq * 4);
  const size_t o_st = io.out(stats, (size_t)nq * 16);
  size_t o_m = 0, o_nm = 0;
  if (merge) { o_m = io.out(merge, (size_t)nq * ccap * 4); o_nm = io.out(nmerge, (size_t)nq * 4); }
  const int rc = orbx::side::upload(p, io);
  if (rc != ORBX_OK) return rc;
  uint8_t* const d = p->io.p;
  c->db = {(const uint32_t*)(d + o_di), (const double*)(d + o_dv), (const int32_t*)(d + o_dn), (const int32_t*)(d + o_map),
           (const int32_t*)(d + o_cov), (float*)(d + o_sc), ndb, db->stride};
  c->q = {(const uint32_t*)(d + o_qi), (const double*)(d + o_qv), (const int32_t*)(d + o_qn), (const int32_t*)(d + o_qm),
          q->d_excl_ptr ? (const int32_t*)(d + o_ep) : nullptr, (const int32_t*)(d + o_ei), nq, q->stride, q->n_excl};
  c->cand = (int32_t*)(d + o_c); c->ncand = (int32_t*)(d + o_nc); c->stats = (int32_t*)(d + o_st);
  c->merge = merge ? (int32_t*)(d + o_m) : nullptr; c->nmerge = merge ? (int32_t*)(d + o_nm) : nullptr;
  return ORBX_OK;
}

}  // namespace
