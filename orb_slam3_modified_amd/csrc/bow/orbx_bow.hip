// The batched bag of words (include/orbx_bow.h): TemplatedVocabulary::transform(features, BowVector&, FeatureVector&, levelsup)
// (TemplatedVocabulary.h:1127-1194) for B frames on descriptors resident in HBM, and L1Scoring::score for all pairs of two batches.
//
// The definition of a frame's result is orbx_bow_finalize (csrc/orbx_matcher.hip), restated here for the device:
//   descent      the product's orbx_bow_transform_device over all nframes * capacity descriptor rows: {word, weight, node} per row
//   k_bowb_frame grid (nframes, 2): workgroup (f, 0) builds frame f's BowVector, workgroup (f, 1) its FeatureVector.  Both compact the kept
//                features (weight > 0) into keys (word << 32 | feature), resp. (node << 32 | feature).  The keys are unique, so ANY sort of
//                them is finalize's stable sort by word: a bitonic network with every comparator pointing up, so that the slots past the
//                keys act as +inf without being stored; in LDS for frames of at most lds_limit features, in the handle's global scratch
//                beyond.  Run heads are counted by a workgroup scan; the thread of a head walks its run and adds the weights in feature
//                order, one __dadd_rn each (double addition is not associative: the order is part of the definition).  The norm is ONE
//                lane walking the compacted values in ascending word order; the division is __ddiv_rn.
//   k_bowb_score grid (ceil(ndb / 256), nq): the query staged in LDS when it fits, one thread per database vector, the sequential merge of
//                k_bow_score_l1.
// The library reads no private state of the vocabulary (see the header): orbx_internal.h is included for orbx::voc_device only.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../orbx_internal.h"
#include "../side/orbx_handle.h"
#include "../side/orbx_pair_device.h"
#include "../../../include/orbx_bow.h"

namespace {

using orbx::side::dev::block_scan;

constexpr int kBowThreads = 512;     // k_bowb_frame: 8 waves
constexpr int kBowLds = 4096;        // keys of one frame sorted in LDS: 32 KiB (a call uses 0 .. kBowLds, ORBX_BOW_LDS; larger frames sort in global memory)
constexpr int kScoreLds = 4000;      // entries of one query staged in LDS: 48 000 bytes (larger queries are read from global memory)

enum { kNormNone = 0, kNormL1 = 1, kNormL2 = 2, kNormCount = 3 };   // kNormCount: DOT_PRODUCT with TF / TF_IDF divides by the number of entries

typedef unsigned long long u64;

// ascending sort of K[0, m): the bitonic network in its one-direction form (the first step of a merge mirrors the upper half), where a
// comparator whose upper end lies at or past m is skipped: that slot stands for +inf and never moves
__device__ __forceinline__ void bowb_cmpx(u64* K, int lo, int hi) {
  const u64 a = K[lo], b = K[hi];
  if (b < a) { K[lo] = b; K[hi] = a; }
}
__device__ __forceinline__ void bowb_sort(u64* K, int m) {
  int lgP = 0;
  while ((1 << lgP) < m) lgP++;
  const int half_pairs = (1 << lgP) >> 1;
  for (int lk = 1; lk <= lgP; lk++) {    // merges of k = 2^lk
    const int lh = lk - 1, h = 1 << lh;
    for (int i = threadIdx.x; i < half_pairs; i += kBowThreads) {
      const int blk = i >> lh, off = i & (h - 1);
      const int lo = (blk << lk) + off, hi = (blk << lk) + (1 << lk) - 1 - off;
      if (hi < m) bowb_cmpx(K, lo, hi);
    }
    __syncthreads();
    for (int lj = lh - 1; lj >= 0; lj--) {
      for (int i = threadIdx.x; i < half_pairs; i += kBowThreads) {
        const int blk = i >> lj, off = i & ((1 << lj) - 1);
        const int lo = (blk << (lj + 1)) + off, hi = lo + (1 << lj);
        if (hi < m) bowb_cmpx(K, lo, hi);
      }
      __syncthreads();
    }
  }
}

struct BowbArgs {
  const uint32_t* word; const double* weight; const uint32_t* node;   // the descent's records, [nframes * cap]
  const int32_t* counts;                                               // [nframes][2]
  u64* gkeys;                                                          // [2][nframes * cap]: the global-memory path's keys
  uint32_t* bow_ids; double* bow_vals; int32_t* bow_n;
  uint32_t* fv_node; int32_t* fv_ptr; uint32_t* fv_feat; int32_t* fv_n;
  int cap, lds_limit, accumulate, norm, part0;
};

// one part (0: BowVector, 1: FeatureVector) of one frame; K holds n keys (LDS or global).  S = K seen as doubles (the values, once the keys
// have been consumed) when STAGE, else the values are summed where they lie in the output.
template <bool STAGE>
__device__ __forceinline__ void bowb_part(const BowbArgs& a, int f, int part, int n, u64* K, int* s_w, int* s_cnt, double* s_norm) {
  const int tid = threadIdx.x, lane = tid & 63;
  const size_t fo = (size_t)f * a.cap;
  // (1) the kept features' keys, in any order
  if (tid == 0) *s_cnt = 0;
  __syncthreads();
  const uint32_t* hi_src = part == 0 ? a.word : a.node;
  for (int i0 = 0; i0 < n; i0 += kBowThreads) {
    const int i = i0 + tid;
    const bool keep = i < n && a.weight[fo + i] > 0;
    const u64 mask = __ballot(keep);
    if (mask) {
      int base = 0;
      const int leader = __ffsll((long long)mask) - 1;
      if (lane == leader) base = atomicAdd(s_cnt, __popcll(mask));
      base = __shfl(base, leader);
      if (keep) K[base + __popcll(mask & ((1ull << lane) - 1ull))] = ((u64)hi_src[fo + i] << 32) | (uint32_t)i;
    }
  }
  __syncthreads();
  const int m = *s_cnt;
  // (2) ascending (word | node, feature)
  bowb_sort(K, m);
  // (3) run heads: thread t owns positions [t * per, (t + 1) * per)
  const int per = (m + kBowThreads - 1) / kBowThreads;
  const int j0 = min(tid * per, m), j1 = min(j0 + per, m);
  int heads = 0;
  for (int j = j0; j < j1; j++) heads += j == 0 || (uint32_t)(K[j] >> 32) != (uint32_t)(K[j - 1] >> 32);
  int k = 0;
  int out = block_scan<kBowThreads / 64>(heads, s_w, &k);   // run heads before this thread's; k = all of them
  if (part == 1) {
    int32_t* ptr = a.fv_ptr + (size_t)f * (a.cap + 1);
    for (int j = j0; j < j1; j++) {
      const u64 key = K[j];
      a.fv_feat[fo + j] = (uint32_t)key;
      if (j == 0 || (uint32_t)(key >> 32) != (uint32_t)(K[j - 1] >> 32)) { a.fv_node[fo + out] = (uint32_t)(key >> 32); ptr[out] = j; out++; }
    }
    if (tid == 0) { ptr[k] = m; a.fv_n[f] = k; }
    return;
  }
  // BowVector::addWeight in feature order (TF_IDF, TF) / addIfNotExist (IDF, BINARY)
  for (int j = j0; j < j1; j++) {
    const u64 key = K[j];
    const uint32_t w = (uint32_t)(key >> 32);
    if (j != 0 && w == (uint32_t)(K[j - 1] >> 32)) continue;
    double acc = a.weight[fo + (uint32_t)key];
    if (a.accumulate)
      for (int q = j + 1; q < m; q++) {
        const u64 kq = K[q];
        if ((uint32_t)(kq >> 32) != w) break;
        acc = __dadd_rn(acc, a.weight[fo + (uint32_t)kq]);
      }
    a.bow_ids[fo + out] = w;
    a.bow_vals[fo + out] = acc;
    out++;
  }
  if (tid == 0) a.bow_n[f] = k;
  if (a.norm == kNormNone || k == 0) return;
  __syncthreads();                       // every run has been read: the keys are dead, the raw values are in the output
  double* vals = a.bow_vals + fo;
  double nrm;
  if (a.norm == kNormCount) nrm = (double)k;
  else {
    const double* S = vals;
    if (STAGE) {
      double* SK = (double*)K;
      for (int j = tid; j < k; j += kBowThreads) SK[j] = vals[j];
      __syncthreads();
      S = SK;
    }
    if (tid == 0) {
      // BowVector::normalize (BowVector.cpp:61-85): one running sum in ascending word order
      double s = 0.0;
      int j = 0;
      if (a.norm == kNormL1) {
        for (; j + 8 <= k; j += 8) {
          double v[8];
#pragma unroll
          for (int u = 0; u < 8; u++) v[u] = S[j + u];
#pragma unroll
          for (int u = 0; u < 8; u++) s = __dadd_rn(s, fabs(v[u]));
        }
        for (; j < k; j++) s = __dadd_rn(s, fabs(S[j]));
      } else {
        for (; j < k; j++) { const double v = S[j]; s = __dadd_rn(s, __dmul_rn(v, v)); }
        s = __dsqrt_rn(s);
      }
      *s_norm = s;
    }
    __syncthreads();
    nrm = *s_norm;
    if (!(nrm > 0.0)) return;
  }
  for (int j = tid; j < k; j += kBowThreads) vals[j] = __ddiv_rn(vals[j], nrm);
}

__global__ __launch_bounds__(kBowThreads) void k_bowb_frame(BowbArgs a) {
  __shared__ u64 s_keys[kBowLds];
  __shared__ int s_w[kBowThreads / 64 + 1];
  __shared__ int s_cnt;
  __shared__ double s_norm;
  const int f = blockIdx.x, part = (int)blockIdx.y + a.part0;
  const int c = a.counts[2 * f];
  if (c < 0) {                           // the quadtree overflow marker: -1 and nothing else
    if (threadIdx.x == 0) { if (part == 0) a.bow_n[f] = -1; else a.fv_n[f] = -1; }
    return;
  }
  const int n = min(c, a.cap);
  if (n <= a.lds_limit) bowb_part<true>(a, f, part, n, s_keys, s_w, &s_cnt, &s_norm);
  else bowb_part<false>(a, f, part, n, a.gkeys + ((size_t)part * gridDim.x + f) * a.cap, s_w, &s_cnt, &s_norm);
}

// one side of the score matrix: vector i = ids / vals + start(i), n(i) entries (fixed stride + counts, or CSR row pointers)
struct BowbSide { const uint32_t* ids; const double* vals; const int32_t* n; const int32_t* ptr; int stride; };
__device__ __forceinline__ void bowb_row(const BowbSide& s, int i, size_t* start, int* n) {
  if (s.ptr) { *start = (size_t)s.ptr[i]; *n = s.ptr[i + 1] - s.ptr[i]; }
  else { *start = (size_t)i * s.stride; *n = min(max(s.n[i], 0), s.stride); }
}

__device__ __forceinline__ double bowb_merge(const uint32_t* qi, const double* qv, int nq, const uint32_t* di, const double* dv, int nd) {
  int x = 0, y = 0;
  double score = 0;
  while (x < nq && y < nd) {
    const uint32_t ia = qi[x], ib = di[y];
    if (ia == ib) {
      const double vi = qv[x], wi = dv[y];
      score = __dadd_rn(score, __dsub_rn(__dsub_rn(fabs(__dsub_rn(vi, wi)), fabs(vi)), fabs(wi)));
      ++x; ++y;
    } else if (ia < ib) ++x;
    else ++y;
  }
  return -score / 2.0;
}

__global__ __launch_bounds__(256) void k_bowb_score(BowbSide q, BowbSide db, int ndb, double* __restrict__ scores) {
  __shared__ uint32_t s_id[kScoreLds];
  __shared__ double s_v[kScoreLds];
  const int qi = blockIdx.y;
  size_t qs; int qn;
  bowb_row(q, qi, &qs, &qn);
  const bool staged = qn <= kScoreLds;   // uniform over the workgroup
  if (staged) {
    for (int j = threadIdx.x; j < qn; j += 256) { s_id[j] = q.ids[qs + j]; s_v[j] = q.vals[qs + j]; }
    __syncthreads();
  }
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= ndb) return;
  size_t ds; int dn;
  bowb_row(db, d, &ds, &dn);
  scores[(size_t)qi * ndb + d] = staged ? bowb_merge(s_id, s_v, qn, db.ids + ds, db.vals + ds, dn)
                                        : bowb_merge(q.ids + qs, q.vals + qs, qn, db.ids + ds, db.vals + ds, dn);
}

}  // namespace

struct orbx_bow : orbx::side::Handle {    // scratch: records [slots] + keys [2][slots]
  orbx_voc* voc = nullptr;
  int levelsup = 0;
  int accumulate = 0, norm = kNormNone;   // learnt from orbx_bow_finalize at create
  int lds_limit = kBowLds;                // ORBX_BOW_LDS at create; h_io: the host forms' fixed-stride results before compaction
};

namespace {

using namespace orbx::side;

struct Scratch { uint32_t* word; double* weight; uint32_t* node; u64* keys; };
size_t scratch_layout(size_t slots, Scratch* s, uint8_t* base) {
  orbx::BlobLayout l;
  const size_t o_wt = l.add(slots * 8), o_k = l.add(slots * 16), o_w = l.add(slots * 4), o_n = l.add(slots * 4);
  if (s) { s->weight = (double*)(base + o_wt); s->keys = (u64*)(base + o_k); s->word = (uint32_t*)(base + o_w); s->node = (uint32_t*)(base + o_n); }
  return l.size;
}

}  // namespace

extern "C" {

int orbx_bow_create(orbx_bow** out, orbx_voc* voc, int levelsup) {
  if (out) *out = nullptr;
  auto bad = [](const char* m, int code = ORBX_E_INVALID) { return create_fail(code, "orbx_bow_create", m); };
  if (!out || !voc) return bad("null argument");
  if (levelsup < 0) return bad("levelsup must be >= 0");
  int nnodes = 0;
  if (orbx_voc_info(voc, nullptr, nullptr, &nnodes, nullptr) != ORBX_OK || nnodes <= 1) return bad("empty vocabulary");
  const int device = orbx::voc_device(voc);
  if (device < 0) return bad("the vocabulary has no device");
  // the weighting's and the scoring's share in a result byte, from the definition itself: features {0, 1} hit word 0 with weight 1 each,
  // feature 2 hits word 1 with weight 2.  Added: {2, 2}, first kept: {1, 2}; then L1: / 4 resp. / 3, L2: / sqrt(8) resp. / sqrt(5),
  // DOT_PRODUCT: {2, 2} / 2 entries resp. {1, 2} untouched.
  const uint32_t pw[3] = {0, 0, 1};
  const double pv[3] = {1.0, 1.0, 2.0};
  uint32_t ids[3];
  double vals[3];
  int pn = 0;
  if (orbx_bow_finalize(voc, pw, pv, 3, ids, vals, &pn) != ORBX_OK || pn != 2) return bad("orbx_bow_finalize failed on the probe");
  const bool added = vals[0] == vals[1];
  int norm;
  if (added) norm = vals[0] == 0.5 ? kNormL1 : vals[0] == 1.0 ? kNormCount : kNormL2;
  else norm = vals[0] == 1.0 ? kNormNone : vals[0] == 1.0 / 3.0 ? kNormL1 : kNormL2;
  if (norm == kNormL2 && vals[0] != (added ? 2.0 / std::sqrt(8.0) : 1.0 / std::sqrt(5.0))) return bad("orbx_bow_finalize gave an unknown normalisation on the probe");
  orbx_bow* b = new orbx_bow();
  b->voc = voc; b->levelsup = levelsup; b->accumulate = added ? 1 : 0; b->norm = norm;
  b->lds_limit = env_int("ORBX_BOW_LDS", 0, kBowLds, kBowLds);
  if (const char* e = open_handle(b, device)) { orbx_bow_destroy(b); return bad(e, ORBX_E_DEVICE); }
  *out = b;
  return ORBX_OK;
}

void orbx_bow_destroy(orbx_bow* b) {
  if (!b) return;
  close_handle(b);
  delete b;
}

const char* orbx_bow_last_error(const orbx_bow* b) { return last_error(b); }

int orbx_bow_transform_batch_device(orbx_bow* b, const uint8_t* d_desc, const int32_t* d_counts, int nframes, int capacity, uint32_t* d_bow_ids,
                                    double* d_bow_vals, int32_t* d_bow_n, uint32_t* d_fv_node, int32_t* d_fv_ptr, uint32_t* d_fv_feat,
                                    int32_t* d_fv_n, void* stream) {
  if (!b) return ORBX_E_INVALID;
  const char* who = "orbx_bow_transform_batch_device: ";
  if (nframes < 1) return fail(b, ORBX_E_INVALID, std::string(who) + "nframes = " + std::to_string(nframes) + " (at least 1)");
  if (capacity < 1) return fail(b, ORBX_E_INVALID, std::string(who) + "capacity = " + std::to_string(capacity) + " (at least 1)");
  if ((long long)nframes * capacity > (long long)INT_MAX) return fail(b, ORBX_E_INVALID, std::string(who) + "nframes * capacity exceeds INT_MAX");
  if (!d_desc || !d_counts) return fail(b, ORBX_E_INVALID, std::string(who) + "null descriptors or counts");
  const int nb = (d_bow_ids != nullptr) + (d_bow_vals != nullptr) + (d_bow_n != nullptr);
  const int nf = (d_fv_node != nullptr) + (d_fv_ptr != nullptr) + (d_fv_feat != nullptr) + (d_fv_n != nullptr);
  if ((nb != 0 && nb != 3) || (nf != 0 && nf != 4)) return fail(b, ORBX_E_INVALID, std::string(who) + "an output group is partly null");
  if (nb == 0 && nf == 0) return fail(b, ORBX_E_INVALID, std::string(who) + "null outputs");
  int rc = same_device(b, who, {d_desc, d_counts, d_bow_ids, d_fv_node}, "the vocabulary");
  if (rc != ORBX_OK) return rc;
  ORBX_SIDE_HIP(b, hipSetDevice(b->device));
  const size_t slots = (size_t)nframes * capacity;
  rc = grow(b, &b->scratch, scratch_layout(slots, nullptr, nullptr));
  if (rc != ORBX_OK) return rc;
  Scratch sc;
  scratch_layout(slots, &sc, b->scratch.p);
  hipStream_t st = stream ? (hipStream_t)stream : b->st;
  if ((rc = wait_previous(b, st)) != ORBX_OK) return rc;
  rc = orbx_bow_transform_device(b->voc, d_desc, (int)slots, b->levelsup, sc.word, sc.weight, sc.node, st);
  if (rc != ORBX_OK) return fail(b, rc, std::string(who) + "the descent failed");
  BowbArgs a;
  a.word = sc.word; a.weight = sc.weight; a.node = sc.node; a.counts = d_counts; a.gkeys = sc.keys;
  a.bow_ids = d_bow_ids; a.bow_vals = d_bow_vals; a.bow_n = d_bow_n;
  a.fv_node = d_fv_node; a.fv_ptr = d_fv_ptr; a.fv_feat = d_fv_feat; a.fv_n = d_fv_n;
  a.cap = capacity; a.lds_limit = b->lds_limit; a.accumulate = b->accumulate; a.norm = b->norm; a.part0 = nb ? 0 : 1;
  hipLaunchKernelGGL(k_bowb_frame, dim3((unsigned)nframes, (nb && nf) ? 2u : 1u), dim3(kBowThreads), 0, st, a);
  return record_call(b, st);
}

int orbx_bow_transform_batch(orbx_bow* b, const uint8_t* desc, const int32_t* counts, int nframes, int capacity, int32_t* bow_ptr, uint32_t* bow_ids,
                             double* bow_vals, int32_t* fv_ptr, uint32_t* fv_node, int32_t* fv_feat_ptr, uint32_t* fv_feat) {
  if (!b) return ORBX_E_INVALID;
  const char* who = "orbx_bow_transform_batch: ";
  if (nframes < 1 || capacity < 1 || (long long)nframes * capacity > (long long)INT_MAX)
    return fail(b, ORBX_E_INVALID, std::string(who) + "nframes and capacity must be at least 1 and their product at most INT_MAX");
  if (!desc || !counts || !bow_ptr || !bow_ids || !bow_vals || !fv_ptr || !fv_node || !fv_feat_ptr || !fv_feat)
    return fail(b, ORBX_E_INVALID, std::string(who) + "null argument");
  const size_t nk = (size_t)nframes * capacity, nfr = (size_t)nframes;
  orbx::BlobLayout io;
  const size_t o_desc = io.add(nk * 32), o_cnt = io.add(nfr * 8);
  const size_t o_out = io.size;          // the results, read back in one copy
  const size_t o_bv = io.add(nk * 8), o_bi = io.add(nk * 4), o_bn = io.add(nfr * 4), o_fn = io.add(nk * 4), o_fp = io.add((nk + nfr) * 4),
               o_ff = io.add(nk * 4), o_fc = io.add(nfr * 4);
  ORBX_SIDE_HIP(b, hipSetDevice(b->device));
  int rc = grow(b, &b->io, io.size);
  if (rc != ORBX_OK) return rc;
  if (b->h_io.size() < io.size - o_out) b->h_io.resize(io.size - o_out);
  uint8_t* d = b->io.p;
  hipStream_t st = b->st;
  ORBX_SIDE_HIP(b, hipMemcpyAsync(d + o_desc, desc, nk * 32, hipMemcpyHostToDevice, st));
  ORBX_SIDE_HIP(b, hipMemcpyAsync(d + o_cnt, counts, nfr * 8, hipMemcpyHostToDevice, st));
  rc = orbx_bow_transform_batch_device(b, d + o_desc, (const int32_t*)(d + o_cnt), nframes, capacity, (uint32_t*)(d + o_bi), (double*)(d + o_bv),
                                       (int32_t*)(d + o_bn), (uint32_t*)(d + o_fn), (int32_t*)(d + o_fp), (uint32_t*)(d + o_ff),
                                       (int32_t*)(d + o_fc), st);
  if (rc != ORBX_OK) return rc;
  uint8_t* h = b->h_io.data();
  ORBX_SIDE_HIP(b, hipMemcpyAsync(h, d + o_out, io.size - o_out, hipMemcpyDeviceToHost, st));
  if ((rc = finish_host(b)) != ORBX_OK) return rc;
  const double* hbv = (const double*)(h + o_bv - o_out);
  const uint32_t* hbi = (const uint32_t*)(h + o_bi - o_out);
  const int32_t* hbn = (const int32_t*)(h + o_bn - o_out);
  const uint32_t* hfn = (const uint32_t*)(h + o_fn - o_out);
  const int32_t* hfp = (const int32_t*)(h + o_fp - o_out);
  const uint32_t* hff = (const uint32_t*)(h + o_ff - o_out);
  const int32_t* hfc = (const int32_t*)(h + o_fc - o_out);
  int nb = 0, nn = 0, nfeat = 0;
  bow_ptr[0] = 0; fv_ptr[0] = 0; fv_feat_ptr[0] = 0;
  for (int f = 0; f < nframes; f++) {
    const size_t fo = (size_t)f * capacity;
    const int kb = std::max(hbn[f], 0), kn = std::max(hfc[f], 0);
    std::memcpy(bow_ids + nb, hbi + fo, sizeof(uint32_t) * kb);
    std::memcpy(bow_vals + nb, hbv + fo, sizeof(double) * kb);
    nb += kb;
    bow_ptr[f + 1] = nb;
    const int32_t* p = hfp + (size_t)f * (capacity + 1);
    for (int j = 0; j < kn; j++) { fv_node[nn + j] = hfn[fo + j]; fv_feat_ptr[nn + j + 1] = nfeat + p[j + 1]; }
    if (kn) { std::memcpy(fv_feat + nfeat, hff + fo, sizeof(uint32_t) * p[kn]); nfeat += p[kn]; }
    nn += kn;
    fv_ptr[f + 1] = nn;
  }
  return ORBX_OK;
}

int orbx_bow_score_matrix_device(orbx_bow* b, const uint32_t* d_q_ids, const double* d_q_vals, const int32_t* d_q_n, int nq, int q_stride,
                                 const uint32_t* d_db_ids, const double* d_db_vals, const int32_t* d_db_n, int ndb, int db_stride, double* d_scores,
                                 void* stream) {
  if (!b) return ORBX_E_INVALID;
  const char* who = "orbx_bow_score_matrix_device: ";
  if (b->norm != kNormL1) return fail(b, ORBX_E_INVALID, std::string(who) + "the vocabulary's vectors do not carry the L1 norm: L1Scoring::score does not apply");
  if (nq < 1 || ndb < 1 || q_stride < 1 || db_stride < 1) return fail(b, ORBX_E_INVALID, std::string(who) + "nq, ndb and the strides must be at least 1");
  if (nq > 65535) return fail(b, ORBX_E_INVALID, std::string(who) + "at most 65535 queries per call");
  if (!d_q_ids || !d_q_vals || !d_q_n || !d_db_ids || !d_db_vals || !d_db_n || !d_scores) return fail(b, ORBX_E_INVALID, std::string(who) + "null buffer");
  int rc = same_device(b, who, {d_q_ids, d_db_ids, d_scores}, "the vocabulary");
  if (rc != ORBX_OK) return rc;
  ORBX_SIDE_HIP(b, hipSetDevice(b->device));
  hipStream_t st = stream ? (hipStream_t)stream : b->st;
  if ((rc = wait_previous(b, st)) != ORBX_OK) return rc;
  const BowbSide q = {d_q_ids, d_q_vals, d_q_n, nullptr, q_stride}, db = {d_db_ids, d_db_vals, d_db_n, nullptr, db_stride};
  hipLaunchKernelGGL(k_bowb_score, dim3((unsigned)((ndb + 255) / 256), (unsigned)nq), dim3(256), 0, st, q, db, ndb, d_scores);
  return record_call(b, st);
}

int orbx_bow_score_matrix(orbx_bow* b, const int32_t* q_ptr, const uint32_t* q_ids, const double* q_vals, int nq, const int32_t* db_ptr,
                          const uint32_t* db_ids, const double* db_vals, int ndb, double* scores) {
  if (!b) return ORBX_E_INVALID;
  const char* who = "orbx_bow_score_matrix: ";
  if (b->norm != kNormL1) return fail(b, ORBX_E_INVALID, std::string(who) + "the vocabulary's vectors do not carry the L1 norm: L1Scoring::score does not apply");
  if (nq < 1 || ndb < 1 || nq > 65535) return fail(b, ORBX_E_INVALID, std::string(who) + "nq must be in [1, 65535] and ndb at least 1");
  if (!q_ptr || !db_ptr || !scores) return fail(b, ORBX_E_INVALID, std::string(who) + "null argument");
  const size_t qz = (size_t)q_ptr[nq], dz = (size_t)db_ptr[ndb];
  if ((qz && (!q_ids || !q_vals)) || (dz && (!db_ids || !db_vals))) return fail(b, ORBX_E_INVALID, std::string(who) + "null argument");
  orbx::BlobLayout io;
  const size_t o_qv = io.add(qz * 8), o_dv = io.add(dz * 8), o_s = io.add((size_t)nq * ndb * 8), o_qi = io.add(qz * 4), o_di = io.add(dz * 4),
               o_qp = io.add(((size_t)nq + 1) * 4), o_dp = io.add(((size_t)ndb + 1) * 4);
  ORBX_SIDE_HIP(b, hipSetDevice(b->device));
  int rc = grow(b, &b->io, io.size);
  if (rc != ORBX_OK) return rc;
  uint8_t* d = b->io.p;
  hipStream_t st = b->st;
  if ((rc = wait_previous(b, st)) != ORBX_OK) return rc;
  if (qz) { ORBX_SIDE_HIP(b, hipMemcpyAsync(d + o_qi, q_ids, qz * 4, hipMemcpyHostToDevice, st)); ORBX_SIDE_HIP(b, hipMemcpyAsync(d + o_qv, q_vals, qz * 8, hipMemcpyHostToDevice, st)); }
  if (dz) { ORBX_SIDE_HIP(b, hipMemcpyAsync(d + o_di, db_ids, dz * 4, hipMemcpyHostToDevice, st)); ORBX_SIDE_HIP(b, hipMemcpyAsync(d + o_dv, db_vals, dz * 8, hipMemcpyHostToDevice, st)); }
  ORBX_SIDE_HIP(b, hipMemcpyAsync(d + o_qp, q_ptr, ((size_t)nq + 1) * 4, hipMemcpyHostToDevice, st));
  ORBX_SIDE_HIP(b, hipMemcpyAsync(d + o_dp, db_ptr, ((size_t)ndb + 1) * 4, hipMemcpyHostToDevice, st));
  const BowbSide q = {(const uint32_t*)(d + o_qi), (const double*)(d + o_qv), nullptr, (const int32_t*)(d + o_qp), 0},
                 db = {(const uint32_t*)(d + o_di), (const double*)(d + o_dv), nullptr, (const int32_t*)(d + o_dp), 0};
  hipLaunchKernelGGL(k_bowb_score, dim3((unsigned)((ndb + 255) / 256), (unsigned)nq), dim3(256), 0, st, q, db, ndb, (double*)(d + o_s));
  ORBX_SIDE_HIP(b, hipGetLastError());
  ORBX_SIDE_HIP(b, hipMemcpyAsync(scores, d + o_s, (size_t)nq * ndb * 8, hipMemcpyDeviceToHost, st));
  return finish_host(b);
}

}  // extern "C"
