// The batched SearchByBoW (include/orbx_match.h): ORBmatcher::SearchByBoW (src/ORBmatcher.cc:223-425 and :765-905, single camera) for P
// (frame, frame) pairs on the descriptors, keypoints and FeatureVectors a batch extraction and orbx_bow_transform_batch_device left in HBM.
//
// k_match_pairs<LDS>: one workgroup of 8 waves per pair (a grid of at most kMaxBlocks workgroups walks the pairs).
//   stage      LDS path: the two descriptor sets by 16-byte LDS-DMA loads, the two fv_feat lists, B's match row (-1 free, -2 an invalid B
//              feature in keyframe mode) -- 36 (capA + capB) + 16 min(capA, capB) + 4 capB bytes; every fv_feat entry is checked against its
//              frame's count on the way.  Global path (pairs that need more LDS than the handle's limit): the same arrays where they lie, the
//              work list and the match row in the handle's scratch (the match row in the caller's d_match_b2a when there is one).
//   intersect  a thread per A node: binary search in B's node list; the common nodes' (a0, a1, b0, b1) ranges are compacted into a work list.
//   nodes      waves take nodes from the list (an LDS counter).  The chain of one node is sequential over its A features and independent of
//              every other node's (a feature sits in one node): no order between waves matters.
//                nb <= wave_node (64): lane j keeps B candidate j -- descriptor in 8 registers, "taken" in one -- over all A features of the
//                  node; the A descriptor is wave-uniform; bestDist1 / first position / bestDist2 are two DPP min-reductions and a ballot.
//                larger: a trip loop, lane j scans candidates j, j + 64, ... with its own (best, position, second); three reductions merge
//                  the lanes: the smallest best, the smallest position among its holders, and the second = min over lanes of (the winner's
//                  second, the others' best) -- the second-smallest of the multiset, ties included.
//              No angle is read here: the rotation histogram needs the bin sizes only, and they are counted afterwards in parallel.
//   filter     after a barrier: a thread per B feature adds its match's bin to an LDS histogram; one lane runs ComputeThreeMaxima; a thread
//              per B feature recomputes its bin, drops the match when the bin lost, writes b2a / a2b and counts.
// Hamming distances range over 0 .. 256: ints everywhere.  256 is also "no candidate": a candidate at distance 256 never passes `< 256`.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <string>

#include "../side/orbx_handle.h"
#include "../side/orbx_pair_device.h"
#include "../side/orbx_pair_host.h"
#include "../../../include/orbx_match.h"

namespace {

using namespace orbx::side::dev;           // ld / st on B's match row: written by one lane, read by the wave's other lanes in the next step

constexpr int kThreads = 512;             // 8 waves

struct Side {
  const uint8_t* kps; const uint8_t* desc; const int32_t* counts; const uint32_t* fv_node; const int32_t* fv_ptr; const uint32_t* fv_feat;
  const int32_t* fv_n; const uint8_t* valid;
  int nframes, cap;
};

struct Args {
  Side a, b;
  const int32_t* pairs;
  int32_t* b2a; int32_t* a2b; int32_t* nm;
  uint8_t* scratch; size_t scratch_stride;   // the global path's work list and match row, one slice per workgroup
  int npairs, th, kf, check_ori, wave_node;
  float ratio;
};

constexpr size_t kAngle = offsetof(orbx_keypoint, angle);

__device__ __forceinline__ void fail_rows(const Args& g, int p, int32_t* ob, int32_t* oa) {
  if (ob) for (int i = threadIdx.x; i < g.b.cap; i += kThreads) ob[i] = -1;
  if (oa) for (int i = threadIdx.x; i < g.a.cap; i += kThreads) oa[i] = -1;
  if (threadIdx.x == 0) g.nm[p] = -1;
}

template <bool LDS>
__global__ __launch_bounds__(kThreads) void k_match_pairs(Args g) {
  extern __shared__ __align__(16) uint8_t smem[];
  __shared__ int s_cnt, s_next, s_bad, s_nm;
  __shared__ int s_hist[32];
  __shared__ int s_ind[3];
  const int tid = threadIdx.x, lane = tid & 63;
  const int capA = g.a.cap, capB = g.b.cap, capW = min(capA, capB);
  // LDS: descriptors A | descriptors B | work list | match row of B | fv_feat A | fv_feat B
  uint8_t* const l_dA = smem;
  uint8_t* const l_dB = smem + (size_t)capA * 32;
  int4* const l_work = (int4*)(smem + (size_t)(capA + capB) * 32);
  int32_t* const l_match = (int32_t*)(l_work + capW);
  uint32_t* const l_fA = (uint32_t*)(l_match + capB);
  uint32_t* const l_fB = l_fA + capA;
  uint8_t* const slice = g.scratch + (size_t)blockIdx.x * g.scratch_stride;

  for (int p = blockIdx.x; p < g.npairs; p += gridDim.x) {
    __syncthreads();                       // the previous pair's shared state has been read
    const int ia = g.pairs[2 * p], ib = g.pairs[2 * p + 1];
    int32_t* const ob = g.b2a ? g.b2a + (size_t)p * capB : nullptr;
    int32_t* const oa = g.a2b ? g.a2b + (size_t)p * capA : nullptr;
    bool ok = ia >= 0 && ia < g.a.nframes && ib >= 0 && ib < g.b.nframes;
    int cA = 0, cB = 0, kA = 0, kB = 0;
    if (ok) {
      cA = g.a.counts[2 * ia]; cB = g.b.counts[2 * ib]; kA = g.a.fv_n[ia]; kB = g.b.fv_n[ib];
      ok = cA >= 0 && cB >= 0 && kA >= 0 && kB >= 0;
    }
    if (!ok) { fail_rows(g, p, ob, oa); continue; }   // uniform over the workgroup
    const int nA = min(cA, capA), nB = min(cB, capB);
    kA = min(kA, capA); kB = min(kB, capB);
    const size_t oA = (size_t)ia * capA, oB = (size_t)ib * capB;
    const int32_t* const pA = g.a.fv_ptr + (size_t)ia * (capA + 1);
    const int32_t* const pB = g.b.fv_ptr + (size_t)ib * (capB + 1);
    const int totA = kA ? clampi(pA[kA], 0, capA) : 0, totB = kB ? clampi(pB[kB], 0, capB) : 0;
    const uint32_t* const gfA = g.a.fv_feat + oA;
    const uint32_t* const gfB = g.b.fv_feat + oB;
    const uint8_t* const vA = g.a.valid ? g.a.valid + oA : nullptr;
    const uint8_t* const vB = (g.kf && g.b.valid) ? g.b.valid + oB : nullptr;
    // this instantiation's arrays: LDS or global, decided at compile time
    const uint8_t* const dA = LDS ? l_dA : g.a.desc + oA * 32;
    const uint8_t* const dB = LDS ? l_dB : g.b.desc + oB * 32;
    const uint32_t* const fA = LDS ? l_fA : gfA;
    const uint32_t* const fB = LDS ? l_fB : gfB;
    int4* const work = LDS ? l_work : (int4*)slice;
    int32_t* const match = LDS ? l_match : (ob ? ob : (int32_t*)(slice + (((size_t)capW * 16 + 15) & ~(size_t)15)));

    // ---- stage and check
    if (tid == 0) { s_cnt = 0; s_next = 0; s_bad = 0; s_nm = 0; }
    if (tid < 32) s_hist[tid] = 0;
    if (LDS) {
      stage_dma<kThreads>(l_dA, g.a.desc + oA * 32, nA * 2);
      stage_dma<kThreads>(l_dB, g.b.desc + oB * 32, nB * 2);
    }
    __syncthreads();                       // s_bad = 0 before anyone raises it
    for (int i = tid; i < totA; i += kThreads) {
      const uint32_t v = gfA[i];
      if (v >= (uint32_t)nA) s_bad = 1;
      if (LDS) l_fA[i] = v;
    }
    for (int i = tid; i < totB; i += kThreads) {
      const uint32_t v = gfB[i];
      if (v >= (uint32_t)nB) s_bad = 1;
      if (LDS) l_fB[i] = v;
    }
    for (int i = tid; i < (LDS ? nB : capB); i += kThreads) match[i] = (i < nB && vB && !vB[i]) ? -2 : -1;
    if (oa) for (int i = tid; i < capA; i += kThreads) oa[i] = -1;
    if (LDS) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the LDS-DMA loads have landed
    __syncthreads();
    if (s_bad) { fail_rows(g, p, ob, oa); continue; }

    // ---- the nodes both frames have
    {
      const uint32_t* const nodeA = g.a.fv_node + oA;
      const uint32_t* const nodeB = g.b.fv_node + oB;
      for (int ja = tid; ja < kA; ja += kThreads) {
        const uint32_t node = nodeA[ja];
        int lo = 0, hi = kB;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (nodeB[mid] < node) lo = mid + 1; else hi = mid;
        }
        if (lo < kB && nodeB[lo] == node) {
          const int a0 = clampi(pA[ja], 0, totA), a1 = clampi(pA[ja + 1], 0, totA);
          const int b0 = clampi(pB[lo], 0, totB), b1 = clampi(pB[lo + 1], 0, totB);
          if (a1 > a0 && b1 > b0) {
            const int k = atomicAdd(&s_cnt, 1);
            if (k < capW) work[k] = make_int4(a0, a1, b0, b1);
          }
        }
      }
    }
    __syncthreads();
    const int nwork = min(s_cnt, capW);

    // ---- one node per wave at a time
    for (;;) {
      const int w = next_work(&s_next);
      if (w >= nwork) break;
      const int4 r = work[w];
      const int a0 = __builtin_amdgcn_readfirstlane(r.x), a1 = __builtin_amdgcn_readfirstlane(r.y);
      const int b0 = __builtin_amdgcn_readfirstlane(r.z), nb = __builtin_amdgcn_readfirstlane(r.w) - b0;
      const int na = a1 - a0;
      const bool regs = nb <= g.wave_node;   // wave-uniform
      uint32_t my_fb = 0;
      bool my_free = false;
      D8 my_db;
#pragma unroll
      for (int k = 0; k < 8; k++) my_db.w[k] = 0;
      if (regs && lane < nb) {
        my_fb = fB[b0 + lane];
        my_free = ld(match + my_fb) == -1;
        my_db = load_desc(dB + (size_t)my_fb * 32);
      }
      for (int c0 = 0; c0 < na; c0 += 64) {
        const int cn = min(64, na - c0);
        int l_fa = 0, l_va = 0;
        if (lane < cn) {
          l_fa = (int)fA[a0 + c0 + lane];
          l_va = vA ? (int)vA[l_fa] : 1;
        }
        for (int i = 0; i < cn; i++) {
          if (!__builtin_amdgcn_readlane(l_va, i)) continue;
          const int fa = __builtin_amdgcn_readlane(l_fa, i);
          const D8 da = load_desc(dA + (size_t)fa * 32);   // wave-uniform address
          if (regs) {
            const int d = my_free ? hamming(da, my_db) : 256;
            const int m = wave_min(d);
            if (m > g.th) continue;
            const int win = __ffsll((long long)__ballot(d == m)) - 1;   // candidates lie in list order over the lanes: the first minimum
            const int d2 = wave_min(lane == win ? 256 : d);
            if ((float)m < g.ratio * (float)d2) {
              if (lane == win) { my_free = false; st(match + my_fb, fa); }
            }
          } else {
            int best = 256, second = 256, pos = INT_MAX;
            uint32_t fbest = 0;
            for (int j = lane; j < nb; j += 64) {
              const uint32_t fb = fB[b0 + j];
              if (ld(match + fb) != -1) continue;
              const int d = hamming(da, load_desc(dB + (size_t)fb * 32));
              if (d < best) { second = best; best = d; pos = j; fbest = fb; }
              else if (d < second) second = d;
            }
            const int m = wave_min(best);
            if (m > g.th) continue;
            const int wpos = wave_min(best == m ? pos : INT_MAX);
            const bool win = best == m && pos == wpos;
            const int d2 = wave_min(win ? second : best);
            if ((float)m < g.ratio * (float)d2) {
              if (win) st(match + fbest, fa);
              __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // the store is done before the next A feature's loads
            }
          }
        }
      }
    }
    __syncthreads();

    // ---- the rotation filter and the outputs
    int i1 = -1, i2 = -1, i3 = -1;
    if (g.check_ori) {
      for (int b = tid; b < nB; b += kThreads) {
        const int m = match[b];
        if (m >= 0) {
          const int bin = rot_bin(kp_field<float>(g.a.kps, oA + m, kAngle), kp_field<float>(g.b.kps, oB + b, kAngle));
          if (bin >= 0) atomicAdd(&s_hist[bin], 1);
        }
      }
      __syncthreads();
      if (tid == 0) {                      // ComputeThreeMaxima, src/ORBmatcher.cc:2012-2053
        int ind1 = -1, ind2 = -1, ind3 = -1, max1 = 0, max2 = 0, max3 = 0;
        for (int i = 0; i < 30; i++) {
          const int s = s_hist[i];
          if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
          else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
          else if (s > max3) { max3 = s; ind3 = i; }
        }
        if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
        else if (max3 < 0.1f * (float)max1) { ind3 = -1; }
        s_ind[0] = ind1; s_ind[1] = ind2; s_ind[2] = ind3;
      }
      __syncthreads();
      i1 = s_ind[0]; i2 = s_ind[1]; i3 = s_ind[2];
    }
    int cnt = 0;
    for (int b = tid; b < capB; b += kThreads) {
      int v = -1;
      if (b < nB) {
        v = match[b];
        if (v >= 0 && g.check_ori) {
          const int bin = rot_bin(kp_field<float>(g.a.kps, oA + v, kAngle), kp_field<float>(g.b.kps, oB + b, kAngle));
          if (bin >= 0 && bin != i1 && bin != i2 && bin != i3) v = -1;
        }
        if (v < 0) v = -1;
      }
      if (ob) ob[b] = v;
      if (v >= 0) {
        if (oa) oa[v] = b;
        cnt++;
      }
    }
    if (cnt) atomicAdd(&s_nm, cnt);
    __syncthreads();
    if (tid == 0) g.nm[p] = s_nm;
  }
}

}  // namespace

struct orbx_match : orbx::side::pair::PairHandle {};   // scratch: per workgroup the global path's work list and match row

namespace {

using namespace orbx::side;
using namespace orbx::side::pair;

Side to_side(const orbx_match_side* s) {
  return {(const uint8_t*)s->d_kps, s->d_desc, s->d_counts, s->d_fv_node, s->d_fv_ptr, s->d_fv_feat, s->d_fv_n, s->d_valid, s->nframes, s->capacity};
}

// what both forms check before anything is copied or launched
int check_call(orbx_match* m, const char* who, const orbx_match_side* a, const orbx_match_side* b, const void* pairs, int npairs, int mode,
               const void* b2a, const void* a2b, const void* nm) {
  int rc = check_sides<true>(m, who, a, b, 0, nullptr, pairs && nm, "pairs or nmatches");
  if (rc != ORBX_OK) return rc;
  if (!b2a && !a2b) return fail(m, ORBX_E_INVALID, std::string(who) + "both match arrays are null");
  if ((rc = check_npairs(m, who, npairs)) != ORBX_OK) return rc;
  if (mode != ORBX_MATCH_FRAME && mode != ORBX_MATCH_KEYFRAMES) return fail(m, ORBX_E_INVALID, std::string(who) + "unknown mode " + std::to_string(mode));
  return check_sizes<true>(m, who, a, b, npairs, std::max(a->capacity, b->capacity), "npairs * capacity");
}

}  // namespace

extern "C" {

int orbx_match_create(orbx_match** out, int device) {
  return create_handle(out, device, "orbx_match_create", orbx_match_destroy, [](orbx_match* m) {
    return open_pair(m, "ORBX_MATCH_LDS", "ORBX_MATCH_WAVE_NODE", (const void*)k_match_pairs<true>);
  });
}

void orbx_match_destroy(orbx_match* m) { destroy_handle(m); }

const char* orbx_match_last_error(const orbx_match* m) { return last_error(m); }

int orbx_match_bow_pairs_device(orbx_match* m, const orbx_match_side* a, const orbx_match_side* b, const int32_t* d_pairs, int npairs, int mode,
                                float nn_ratio, int check_orientation, int32_t* d_match_b2a, int32_t* d_match_a2b, int32_t* d_nmatches,
                                void* stream) {
  if (!m) return ORBX_E_INVALID;
  const char* who = "orbx_match_bow_pairs_device: ";
  int rc = check_call(m, who, a, b, d_pairs, npairs, mode, d_match_b2a, d_match_a2b, d_nmatches);
  if (rc != ORBX_OK) return rc;
  rc = same_device(m, who, {a->d_kps, a->d_desc, a->d_fv_feat, b->d_kps, b->d_desc, b->d_fv_feat, d_pairs, d_match_b2a, d_match_a2b, d_nmatches}, "the handle");
  if (rc != ORBX_OK) return rc;
  ORBX_SIDE_HIP(m, hipSetDevice(m->device));
  const size_t capA = (size_t)a->capacity, capB = (size_t)b->capacity, capW = std::min(capA, capB);
  const size_t lds = 32 * (capA + capB) + 16 * capW + 4 * (capB + capA + capB);
  Args g;
  g.a = to_side(a); g.b = to_side(b);
  g.pairs = d_pairs; g.b2a = d_match_b2a; g.a2b = d_match_a2b; g.nm = d_nmatches;
  g.npairs = npairs; g.th = mode == ORBX_MATCH_KEYFRAMES ? 49 : 50; g.kf = mode == ORBX_MATCH_KEYFRAMES; g.check_ori = check_orientation != 0;
  g.wave_node = m->wave_node; g.ratio = nn_ratio;
  return launch(m, lds <= (size_t)m->lds_limit, lds, (((capW * 16 + 15) & ~(size_t)15) + capB * 4 + 255) & ~(size_t)255, std::min(npairs, kMaxBlocks),
                kThreads, g, k_match_pairs<true>, k_match_pairs<false>, stream);
}

int orbx_match_bow_pairs(orbx_match* m, const orbx_match_side* a, const orbx_match_side* b, const int32_t* pairs, int npairs, int mode, float nn_ratio,
                         int check_orientation, int32_t* match_b2a, int32_t* match_a2b, int32_t* nmatches) {
  if (!m) return ORBX_E_INVALID;
  const char* who = "orbx_match_bow_pairs: ";
  int rc = check_call(m, who, a, b, pairs, npairs, mode, match_b2a, match_a2b, nmatches);
  if (rc != ORBX_OK) return rc;
  const auto arrays = side_arrays<true, orbx_match_side>({{offsetof(orbx_match_side, d_valid), 0, 1, true}});
  Stager io;
  const StagedSides off = stage_sides(io, a, b, arrays);
  const size_t o_pairs = io.in(pairs, (size_t)npairs * 8);
  const size_t o_b2a = io.out(match_b2a, (size_t)npairs * b->capacity * 4), o_a2b = io.out(match_a2b, (size_t)npairs * a->capacity * 4),
               o_nm = io.out(nmatches, (size_t)npairs * 4);
  if ((rc = upload(m, io)) != ORBX_OK) return rc;
  uint8_t* d = m->io.p;
  orbx_match_side ds[2];
  device_sides(d, off, a, b, arrays, ds);
  rc = orbx_match_bow_pairs_device(m, &ds[0], &ds[1], (const int32_t*)(d + o_pairs), npairs, mode, nn_ratio, check_orientation, (int32_t*)(d + o_b2a),
                                   (int32_t*)(d + o_a2b), (int32_t*)(d + o_nm), m->st);
  if (rc != ORBX_OK) return rc;
  return download(m, io);
}

}  // extern "C"
