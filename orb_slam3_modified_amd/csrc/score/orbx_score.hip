// All six DBoW2 scorings for every (query, database) pair of two batches of BowVectors (include/orbx_score.h,
// Thirdparty/DBoW2/DBoW2/ScoringObject.cpp).  The specification is orbx_score_pair below, the reference's loops as C on the host; the device
// computes five of them (KL needs glibc's log bit for bit: host only).
//
// k_score<SCORING>, one instantiation per scoring, grid nq * ceil(ndb / 32), workgroups of 8 waves:
//   a workgroup owns one query and a tile of 32 database vectors, A WAVE PER PAIR (four pairs a wave, one after the other).
//   The query's ids and values are staged once per workgroup in LDS, by 16-byte loads: the LDS image keeps the row's offset inside its
//   16-byte line, so that an aligned global chunk is an aligned LDS chunk; the row's ragged ends go entry by entry.  A query of more than
//   lds_limit entries (at most 4096: 48 KiB) is read where it lies.
//   The intersection is found in parallel: the wave's lanes stride over the database vector's entries (64 consecutive ids a load:
//   coalesced) and each binary-searches the query for its id; a hit computes its term, every operation rounded once (__dmul_rn,
//   __ddiv_rn, __dsqrt_rn; the file is built with -ffp-contract=off).
//   Only the sum is ordered.  The lanes of one stride hold ascending word ids, so the ballot of the hits IS the compaction: the terms are
//   taken out of the hit lanes in ascending lane order (v_readlane with the lane index counted out of the ballot mask) and added to a
//   running sum that is uniform over the wave -- the additions of the reference's walk, in its order, starting from 0.  Lane 0 stores.
// No scratch memory, no inline assembly, no atomics; nothing depends on scheduling.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>

#include "../side/orbx_bowvec_device.h"
#include "../side/orbx_handle.h"
#include "../../../include/orbx_score.h"

namespace {

constexpr int kScoreLds = 4096;           // entries of one query staged in LDS: 16 KiB of ids, 32 KiB of values (ORBX_SCORE_LDS lowers it)
constexpr int kWaves = 8;                 // waves of a workgroup
constexpr int kThreads = kWaves * 64;
constexpr int kTile = 32;                 // database vectors of a workgroup
static_assert(kTile % kWaves == 0, "every wave the same number of pairs");

enum : int { kL1 = ORBX_SCORE_L1_NORM, kL2 = ORBX_SCORE_L2_NORM, kChi = ORBX_SCORE_CHI_SQUARE, kKL = ORBX_SCORE_KL,
             kBha = ORBX_SCORE_BHATTACHARYYA, kDot = ORBX_SCORE_DOT_PRODUCT };

using orbx::side::Side;
using orbx::side::side_row;

// the term of one common word; false: the word adds nothing (CHI_SQUARE's vi + wi == 0)
template <int S>
__device__ __forceinline__ bool score_term(double vi, double wi, double* t) {
  if (S == kL1) { *t = __dsub_rn(__dsub_rn(fabs(__dsub_rn(vi, wi)), fabs(vi)), fabs(wi)); return true; }
  if (S == kChi) {
    const double sum = __dadd_rn(vi, wi);
    *t = __ddiv_rn(__dmul_rn(vi, wi), sum);
    return sum != 0.0;
  }
  if (S == kBha) { *t = __dsqrt_rn(__dmul_rn(vi, wi)); return true; }
  *t = __dmul_rn(vi, wi);                 // L2_NORM, DOT_PRODUCT
  return true;
}

template <int S>
__device__ __forceinline__ double score_finish(double score) {
  if (S == kL1) return -score / 2.0;
  if (S == kL2) return score >= 1 ? 1.0 : __dsub_rn(1.0, __dsqrt_rn(__dsub_rn(1.0, score)));
  if (S == kChi) return __dmul_rn(2., score);
  return score;
}

// One pair by one wave: the sum over the common words in ascending id, the same value in every lane.  qi / qv: the query (LDS or global),
// di / dv: the database vector (global).
template <int S>
__device__ __forceinline__ double score_pair_wave(const uint32_t* qi, const double* qv, int qn, const uint32_t* di, const double* dv, int dn,
                                                  int lane) {
  double score = 0;
  for (int base = 0; base < dn; base += 64) {
    const int j = base + lane;
    bool hit = false;
    double t = 0;
    if (j < dn) {
      const uint32_t id = di[j];
      const int lo = orbx::side::first_not_below(qi, qn, id);
      if (lo < qn && qi[lo] == id) hit = score_term<S>(qv[lo], dv[j], &t);
    }
    unsigned long long m = __ballot(hit);
    const int thi = __double2hiint(t), tlo = __double2loint(t);
    while (m) {                           // uniform over the wave: ascending lane = ascending word id
      const int l = __builtin_ctzll(m);
      m &= m - 1;
      score = __dadd_rn(score, __hiloint2double(__builtin_amdgcn_readlane(thi, l), __builtin_amdgcn_readlane(tlo, l)));
    }
  }
  return score;
}

template <int S>
__global__ __launch_bounds__(kThreads) void k_score(Side q, Side db, int ndb, int tiles, int lds_limit, double* __restrict__ scores) {
  __shared__ __align__(16) uint32_t s_id[kScoreLds + 4];   // the row's image from its 16-byte line on: entry j at [j + mi]
  __shared__ __align__(16) double s_v[kScoreLds + 2];      // entry j at [j + mv]
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
    int dn;
    side_row(db, d, &ds, &dn);
    const double sum = staged ? score_pair_wave<S>(s_id + mi, s_v + mv, qn, db.ids + ds, db.vals + ds, dn, lane)
                              : score_pair_wave<S>(gi, gv, qn, db.ids + ds, db.vals + ds, dn, lane);
    if (lane == 0) scores[(size_t)qidx * ndb + d] = score_finish<S>(sum);
  }
}

// GeneralScoring::LOG_EPS (ScoringObject.cpp:18): libm's log at load time, as the reference's static initialiser evaluates it
const volatile double kDblEpsilon = DBL_EPSILON;
const double kLogEps = std::log(kDblEpsilon);

// the reference's walks over sorted vectors with unique ids: its lower_bound jumps land where a linear merge arrives
template <class F>
inline void for_common(const uint32_t* ida, const double* va, int na, const uint32_t* idb, const double* vb, int nb, F f) {
  int x = 0, y = 0;
  while (x < na && y < nb) {
    if (ida[x] == idb[y]) { f(va[x], vb[y]); ++x; ++y; }
    else if (ida[x] < idb[y]) ++x;
    else ++y;
  }
}

}  // namespace

struct orbx_score : orbx::side::Handle {
  int lds_limit = kScoreLds;              // ORBX_SCORE_LDS at create
};

namespace {

using namespace orbx::side;

void launch(int scoring, hipStream_t st, const Side& q, const Side& db, int nq, int ndb, int lds_limit, double* d_scores) {
  const int tiles = (ndb + kTile - 1) / kTile;
  const dim3 grid((unsigned)nq * (unsigned)tiles), block(kThreads);     // nq * tiles <= nq * ndb <= INT_MAX
  switch (scoring) {
    case kL1: hipLaunchKernelGGL(k_score<kL1>, grid, block, 0, st, q, db, ndb, tiles, lds_limit, d_scores); break;
    case kL2: hipLaunchKernelGGL(k_score<kL2>, grid, block, 0, st, q, db, ndb, tiles, lds_limit, d_scores); break;
    case kChi: hipLaunchKernelGGL(k_score<kChi>, grid, block, 0, st, q, db, ndb, tiles, lds_limit, d_scores); break;
    case kBha: hipLaunchKernelGGL(k_score<kBha>, grid, block, 0, st, q, db, ndb, tiles, lds_limit, d_scores); break;
    default: hipLaunchKernelGGL(k_score<kDot>, grid, block, 0, st, q, db, ndb, tiles, lds_limit, d_scores); break;
  }
}

// what both matrix forms check first
int check_matrix(orbx_score* s, const std::string& who, int scoring, int nq, int ndb) {
  if (scoring < 0 || scoring > 5) return fail(s, ORBX_E_INVALID, who + "scoring = " + std::to_string(scoring) + " (DBoW2's ScoringType, 0 .. 5)");
  if (scoring == kKL)
    return fail(s, ORBX_E_INVALID, who + "KL is host only (orbx_score_pair): vi * log(vi / wi) needs glibc's double log bit for bit, which the device cannot restate");
  if (nq < 1 || ndb < 1) return fail(s, ORBX_E_INVALID, who + "nq and ndb must be at least 1");
  if ((long long)nq * (long long)ndb > (long long)INT_MAX) return fail(s, ORBX_E_INVALID, who + "nq * ndb exceeds INT_MAX");
  return ORBX_OK;
}

bool ascending(const int32_t* p, int n) {
  if (p[0] < 0) return false;
  for (int i = 0; i < n; i++)
    if (p[i + 1] < p[i]) return false;
  return true;
}

}  // namespace

extern "C" {

int orbx_score_create(orbx_score** out, int device) {
  return create_handle(out, device, "orbx_score_create", orbx_score_destroy, [](orbx_score* s) {
    s->lds_limit = env_int("ORBX_SCORE_LDS", 0, kScoreLds, kScoreLds);
    return (const char*)nullptr;
  });
}

void orbx_score_destroy(orbx_score* s) { destroy_handle(s); }

const char* orbx_score_last_error(const orbx_score* s) { return last_error(s); }

double orbx_score_pair(int scoring, const uint32_t* ida, const double* va, int na, const uint32_t* idb, const double* vb, int nb) {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  na = std::max(na, 0); nb = std::max(nb, 0);
  if (scoring < 0 || scoring > 5 || (na && (!ida || !va)) || (nb && (!idb || !vb))) return nan;
  double score = 0;
  switch (scoring) {
    case kL1:
      for_common(ida, va, na, idb, vb, nb, [&](double vi, double wi) { score += std::fabs(vi - wi) - std::fabs(vi) - std::fabs(wi); });
      return -score / 2.0;
    case kL2:
      for_common(ida, va, na, idb, vb, nb, [&](double vi, double wi) { score += vi * wi; });
      return score >= 1 ? 1.0 : 1.0 - std::sqrt(1.0 - score);
    case kChi:
      for_common(ida, va, na, idb, vb, nb, [&](double vi, double wi) { if (vi + wi != 0.0) score += vi * wi / (vi + wi); });
      return 2. * score;
    case kBha:
      for_common(ida, va, na, idb, vb, nb, [&](double vi, double wi) { score += std::sqrt(vi * wi); });
      return score;
    case kDot:
      for_common(ida, va, na, idb, vb, nb, [&](double vi, double wi) { score += vi * wi; });
      return score;
    default: break;
  }
  // KL (:175-221): the first vector advances ONE entry at a time, and each of its words the second lacks adds a term
  int x = 0, y = 0;
  while (x < na && y < nb) {
    const double vi = va[x], wi = vb[y];
    if (ida[x] == idb[y]) {
      if (vi != 0 && wi != 0) score += vi * std::log(vi / wi);
      ++x; ++y;
    } else if (ida[x] < idb[y]) {
      score += vi * (std::log(vi) - kLogEps);     // no test of vi here
      ++x;
    } else {
      ++y;                                        // = lower_bound(ida[x]) when it is reached again
    }
  }
  for (; x < na; ++x)
    if (va[x] != 0) score += va[x] * (std::log(va[x]) - kLogEps);
  return score;
}

int orbx_score_matrix_device(orbx_score* s, int scoring, const uint32_t* d_q_ids, const double* d_q_vals, const int32_t* d_q_n, int nq, int q_stride,
                             const uint32_t* d_db_ids, const double* d_db_vals, const int32_t* d_db_n, int ndb, int db_stride, double* d_scores,
                             void* stream) {
  if (!s) return ORBX_E_INVALID;
  const std::string who = "orbx_score_matrix_device: ";
  int rc = check_matrix(s, who, scoring, nq, ndb);
  if (rc != ORBX_OK) return rc;
  if (q_stride < 1 || db_stride < 1) return fail(s, ORBX_E_INVALID, who + "the strides must be at least 1");
  if (!d_q_ids || !d_q_vals || !d_q_n || !d_db_ids || !d_db_vals || !d_db_n || !d_scores) return fail(s, ORBX_E_INVALID, who + "null buffer");
  rc = same_device(s, who.c_str(), {d_q_ids, d_q_vals, d_q_n, d_db_ids, d_db_vals, d_db_n, d_scores}, "the handle");
  if (rc != ORBX_OK) return rc;
  ORBX_SIDE_HIP(s, hipSetDevice(s->device));
  hipStream_t st = stream ? (hipStream_t)stream : s->st;
  if ((rc = wait_previous(s, st)) != ORBX_OK) return rc;
  const Side q = {d_q_ids, d_q_vals, d_q_n, nullptr, q_stride}, db = {d_db_ids, d_db_vals, d_db_n, nullptr, db_stride};
  launch(scoring, st, q, db, nq, ndb, s->lds_limit, d_scores);
  return record_call(s, st);
}

int orbx_score_matrix(orbx_score* s, int scoring, const int32_t* q_ptr, const uint32_t* q_ids, const double* q_vals, int nq, const int32_t* db_ptr,
                      const uint32_t* db_ids, const double* db_vals, int ndb, double* scores) {
  if (!s) return ORBX_E_INVALID;
  const std::string who = "orbx_score_matrix: ";
  int rc = check_matrix(s, who, scoring, nq, ndb);
  if (rc != ORBX_OK) return rc;
  if (!q_ptr || !db_ptr || !scores) return fail(s, ORBX_E_INVALID, who + "null argument");
  if (!ascending(q_ptr, nq) || !ascending(db_ptr, ndb)) return fail(s, ORBX_E_INVALID, who + "a row pointer begins below 0 or descends");
  const size_t qz = (size_t)q_ptr[nq], dz = (size_t)db_ptr[ndb];
  if ((qz && (!q_ids || !q_vals)) || (dz && (!db_ids || !db_vals))) return fail(s, ORBX_E_INVALID, who + "null argument");
  Stager io;
  size_t o_qv = 0, o_qi = 0, o_dv = 0, o_di = 0;
  if (qz) { o_qv = io.in(q_vals, qz * 8); o_qi = io.in(q_ids, qz * 4); }
  if (dz) { o_dv = io.in(db_vals, dz * 8); o_di = io.in(db_ids, dz * 4); }
  const size_t o_qp = io.in(q_ptr, ((size_t)nq + 1) * 4), o_dp = io.in(db_ptr, ((size_t)ndb + 1) * 4);
  const size_t o_s = io.out(scores, (size_t)nq * ndb * 8);
  if ((rc = upload(s, io)) != ORBX_OK) return rc;
  uint8_t* const d = s->io.p;
  const Side q = {(const uint32_t*)(d + o_qi), (const double*)(d + o_qv), nullptr, (const int32_t*)(d + o_qp), 0},
             db = {(const uint32_t*)(d + o_di), (const double*)(d + o_dv), nullptr, (const int32_t*)(d + o_dp), 0};
  launch(scoring, s->st, q, db, nq, ndb, s->lds_limit, (double*)(d + o_s));
  ORBX_SIDE_HIP(s, hipGetLastError());
  return download(s, io);
}

}  // extern "C"
