// The two-camera rig block of SearchByBoW, batched, and the stacked rig frame it runs on (include/orbx_rigbow.h): ORBmatcher::SearchByBoW
// (src/ORBmatcher.cc:223-425 with F.Nleft != -1, :765-905 with NLeft != -1) for P (frame, frame) pairs on stacked descriptors, keypoints and
// FeatureVectors in HBM.
//
// k_rigbow_stack: one launch for all frames, blockIdx.y the frame.  The counts are read on the device; a thread per 16-byte descriptor piece
//   and per 4-byte keypoint word of the stacked row picks its source (left, right at row - nl, or zero).
// k_rigbow_pairs<LDS>: k_match_pairs' shape (csrc/match/orbx_match.hip), one workgroup of 8 waves per pair.
//   stage      LDS path: B alone -- its descriptors by 16-byte LDS-DMA loads, its fv_feat list, its match row (-1 free, -2 no candidate: in
//              keyframes mode a B feature with valid 0 or at nleft and beyond) and the work list packed to 8 bytes a node: 40 capB + 8 min(capA,
//              capB) bytes.  A's descriptors are read once per query at a wave-uniform address and its fv_feat once per node: where they lie.
//              Global path: everything where it lies, the work list (16 bytes a node) and the match row in the handle's scratch (the match
//              row in the caller's d_match_b2a when there is one).  Every fv_feat entry is checked against its frame's count on the way.
//   intersect  a thread per A node: binary search in B's node list (copied from k_match_pairs).
//   nodes      waves take nodes from the list.  Per query two masked reductions over one candidate set: left (minimum, first position,
//              second) and right (minimum, first position); both are finished before either winner is bound, so both see one snapshot.
//                nb <= wave_node (64): lane j keeps candidate j -- descriptor in 8 registers, its camera and its free bit.
//                larger: the trip loop, lane j scans candidates j, j + 64, ... with (best, position, second) and (bestR, positionR).
//   filter     after a barrier, over B slots: a slot's bin from its holder's angle and its own; ComputeThreeMaxima (copied); a slot of a
//              losing bin is cleared; a2b's column is the slot's camera.
// Hamming distances range over 0 .. 256: ints everywhere.  256 is also "no candidate".
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <string>

#include "../side/orbx_handle.h"
#include "../side/orbx_pair_device.h"
#include "../side/orbx_pair_host.h"
#include "../../../include/orbx_rigbow.h"

namespace {

using namespace orbx::side::dev;

constexpr int kThreads = 512;             // 8 waves
constexpr int kPackedCap = 65535;         // the LDS work list keeps a range's ends in 16 bits
constexpr int kStackThreads = 256;

struct Side {
  const uint8_t* kps; const uint8_t* desc; const int32_t* counts; const uint32_t* fv_node; const int32_t* fv_ptr; const uint32_t* fv_feat;
  const int32_t* fv_n; const uint8_t* valid; const int32_t* nleft;
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

struct StackArgs {
  const uint32_t* kps_l; const uint4* desc_l; const int32_t* counts_l;
  const uint32_t* kps_r; const uint4* desc_r; const int32_t* counts_r;
  uint32_t* kps_s; uint4* desc_s; int32_t* counts_s; int32_t* nleft;
  int cap_l, cap_r, cap_s;
};

constexpr size_t kAngle = offsetof(orbx_keypoint, angle);
constexpr int kKpWords = (int)(sizeof(orbx_keypoint) / 4);
static_assert(sizeof(orbx_keypoint) == 28, "a keypoint is seven words");

__global__ __launch_bounds__(kStackThreads) void k_rigbow_stack(StackArgs g) {
  const int f = blockIdx.y;
  int nl = g.counts_l[2 * f], nr = g.counts_r[2 * f];
  const bool ok = nl >= 0 && nl <= g.cap_l && nr >= 0 && nr <= g.cap_r && nr <= g.cap_s - nl;
  if (!ok) { nl = 0; nr = 0; }             // zero rows; nothing of the frame is read
  const int n = nl + nr;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    g.counts_s[2 * f] = ok ? n : -1; g.counts_s[2 * f + 1] = 0;
    g.nleft[f] = ok ? nl : -1;
  }
  const int step = gridDim.x * kStackThreads, t0 = blockIdx.x * kStackThreads + threadIdx.x;
  const uint4* const dl = g.desc_l + (size_t)f * g.cap_l * 2;
  const uint4* const dr = g.desc_r + (size_t)f * g.cap_r * 2;
  uint4* const ds = g.desc_s + (size_t)f * g.cap_s * 2;
  for (int i = t0; i < g.cap_s * 2; i += step) {
    const int row = i >> 1;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (row < nl) v = dl[i];
    else if (row < n) v = dr[i - 2 * nl];
    ds[i] = v;
  }
  const uint32_t* const kl = g.kps_l + (size_t)f * g.cap_l * kKpWords;
  const uint32_t* const kr = g.kps_r + (size_t)f * g.cap_r * kKpWords;
  uint32_t* const ks = g.kps_s + (size_t)f * g.cap_s * kKpWords;
  for (int i = t0; i < g.cap_s * kKpWords; i += step) {
    const int row = i / kKpWords;
    uint32_t v = 0;
    if (row < nl) v = kl[i];
    else if (row < n) v = kr[i - kKpWords * nl];
    ks[i] = v;
  }
}

__device__ __forceinline__ void fail_rows(const Args& g, int p, int32_t* ob, int32_t* oa) {
  if (ob) for (int i = threadIdx.x; i < g.b.cap; i += kThreads) ob[i] = -1;
  if (oa) for (int i = threadIdx.x; i < 2 * g.a.cap; i += kThreads) oa[i] = -1;
  if (threadIdx.x == 0) g.nm[p] = -1;
}

template <bool LDS>
__global__ __launch_bounds__(kThreads) void k_rigbow_pairs(Args g) {
  extern __shared__ __align__(16) uint8_t smem[];
  __shared__ int s_cnt, s_next, s_bad, s_nm;
  __shared__ int s_hist[32];
  __shared__ int s_ind[3];
  const int tid = threadIdx.x, lane = tid & 63;
  const int capA = g.a.cap, capB = g.b.cap, capW = min(capA, capB);
  // LDS: descriptors B | match row of B | fv_feat B | work list (two packed words a node)
  uint8_t* const l_dB = smem;
  int32_t* const l_match = (int32_t*)(smem + (size_t)capB * 32);
  uint32_t* const l_fB = (uint32_t*)(l_match + capB);
  uint2* const l_work = (uint2*)(l_fB + capB);
  uint8_t* const slice = g.scratch + (size_t)blockIdx.x * g.scratch_stride;

  for (int p = blockIdx.x; p < g.npairs; p += gridDim.x) {
    __syncthreads();                       // the previous pair's shared state has been read
    const int ia = g.pairs[2 * p], ib = g.pairs[2 * p + 1];
    int32_t* const ob = g.b2a ? g.b2a + (size_t)p * capB : nullptr;
    int32_t* const oa = g.a2b ? g.a2b + (size_t)p * capA * 2 : nullptr;
    bool ok = ia >= 0 && ia < g.a.nframes && ib >= 0 && ib < g.b.nframes;
    int cA = 0, cB = 0, kA = 0, kB = 0, nlA = -1, nlB = -1;
    if (ok) {
      cA = g.a.counts[2 * ia]; cB = g.b.counts[2 * ib]; kA = g.a.fv_n[ia]; kB = g.b.fv_n[ib];
      if (g.a.nleft) nlA = g.a.nleft[ia];
      if (g.b.nleft) nlB = g.b.nleft[ib];
      ok = cA >= 0 && cB >= 0 && kA >= 0 && kB >= 0 && nlA >= -1 && nlA <= cA && nlB >= -1 && nlB <= cB;
    }
    if (!ok) { fail_rows(g, p, ob, oa); continue; }   // uniform over the workgroup
    const int nA = min(cA, capA), nB = min(cB, capB);
    kA = min(kA, capA); kB = min(kB, capB);
    const size_t oA = (size_t)ia * capA, oB = (size_t)ib * capB;
    const int32_t* const pA = g.a.fv_ptr + (size_t)ia * (capA + 1);
    const int32_t* const pB = g.b.fv_ptr + (size_t)ib * (capB + 1);
    const int totA = kA ? clampi(pA[kA], 0, capA) : 0, totB = kB ? clampi(pB[kB], 0, capB) : 0;
    const uint32_t* const fA = g.a.fv_feat + oA;
    const uint32_t* const gfB = g.b.fv_feat + oB;
    const uint8_t* const vA = g.a.valid ? g.a.valid + oA : nullptr;
    const uint8_t* const vB = (g.kf && g.b.valid) ? g.b.valid + oB : nullptr;
    const int queryEnd = (g.kf && nlA >= 0) ? nlA : INT_MAX;   // keyframes mode, :800: A features from here on are no queries
    const int candEnd = (g.kf && nlB >= 0) ? nlB : INT_MAX;    // keyframes mode, :820: B features from here on are no candidates
    const int split = (!g.kf && nlB >= 0) ? nlB : INT_MAX;     // frame mode: B features from here on are the right camera's
    const bool rig = split != INT_MAX;                         // frame mode only: there g.th is TH_LOW, the right accept's bound too (:357)
    const uint8_t* const dA = g.a.desc + oA * 32;
    // this instantiation's arrays of B: LDS or global, decided at compile time
    const uint8_t* const dB = LDS ? l_dB : g.b.desc + oB * 32;
    const uint32_t* const fB = LDS ? l_fB : gfB;
    int4* const g_work = (int4*)slice;
    int32_t* const match = LDS ? l_match : (ob ? ob : (int32_t*)(slice + (((size_t)capW * 16 + 15) & ~(size_t)15)));

    // ---- stage and check
    if (tid == 0) { s_cnt = 0; s_next = 0; s_bad = 0; s_nm = 0; }
    if (tid < 32) s_hist[tid] = 0;
    if (LDS) stage_dma<kThreads>(l_dB, g.b.desc + oB * 32, nB * 2);
    __syncthreads();                       // s_bad = 0 before anyone raises it
    for (int i = tid; i < totA; i += kThreads)
      if (fA[i] >= (uint32_t)nA) s_bad = 1;
    for (int i = tid; i < totB; i += kThreads) {
      const uint32_t v = gfB[i];
      if (v >= (uint32_t)nB) s_bad = 1;
      if (LDS) l_fB[i] = v;
    }
    for (int i = tid; i < (LDS ? nB : capB); i += kThreads) match[i] = (i < nB && ((vB && !vB[i]) || i >= candEnd)) ? -2 : -1;
    if (oa) for (int i = tid; i < 2 * capA; i += kThreads) oa[i] = -1;
    if (LDS) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the LDS-DMA loads have landed
    __syncthreads();
    if (s_bad) { fail_rows(g, p, ob, oa); continue; }

    // ---- the nodes both frames have (k_match_pairs' intersection)
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
            if (k < capW) {
              if (LDS) l_work[k] = make_uint2((uint32_t)a0 | ((uint32_t)a1 << 16), (uint32_t)b0 | ((uint32_t)b1 << 16));   // capacities <= 65535
              else g_work[k] = make_int4(a0, a1, b0, b1);
            }
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
      int4 r;
      if (LDS) { const uint2 q = l_work[w]; r = make_int4((int)(q.x & 0xffffu), (int)(q.x >> 16), (int)(q.y & 0xffffu), (int)(q.y >> 16)); }
      else r = g_work[w];
      const int a0 = __builtin_amdgcn_readfirstlane(r.x), a1 = __builtin_amdgcn_readfirstlane(r.y);
      const int b0 = __builtin_amdgcn_readfirstlane(r.z), nb = __builtin_amdgcn_readfirstlane(r.w) - b0;
      const int na = a1 - a0;
      const bool regs = nb <= g.wave_node;   // wave-uniform
      uint32_t my_fb = 0;
      bool my_free = false, my_right = false;
      D8 my_db;
#pragma unroll
      for (int k = 0; k < 8; k++) my_db.w[k] = 0;
      if (regs && lane < nb) {
        my_fb = fB[b0 + lane];
        my_free = ld(match + my_fb) == -1;
        my_right = my_fb >= (uint32_t)split;
        my_db = load_desc(dB + (size_t)my_fb * 32);
      }
      for (int c0 = 0; c0 < na; c0 += 64) {
        const int cn = min(64, na - c0);
        int l_fa = 0, l_va = 0;
        if (lane < cn) {
          l_fa = (int)fA[a0 + c0 + lane];
          l_va = (vA ? (int)vA[l_fa] : 1) && l_fa < queryEnd;
        }
        for (int i = 0; i < cn; i++) {
          if (!__builtin_amdgcn_readlane(l_va, i)) continue;
          const int fa = __builtin_amdgcn_readlane(l_fa, i);
          const D8 da = load_desc(dA + (size_t)fa * 32);   // wave-uniform address
          if (regs) {
            const int d = my_free ? hamming(da, my_db) : 256;
            const int dl = my_right ? 256 : d;
            const int m = wave_min(dl);
            if (m > g.th) continue;        // no right binding either: the right accept is nested in the left distance test
            const int win = __ffsll((long long)__ballot(dl == m)) - 1;   // candidates lie in list order over the lanes: the first minimum
            const int d2 = wave_min(lane == win ? 256 : dl);
            int winr = -1;
            if (rig) {
              const int dr = my_right ? d : 256;
              const int mr = wave_min(dr);
              if (mr <= g.th) winr = __ffsll((long long)__ballot(dr == mr)) - 1;
            }
            const bool left = (float)m < g.ratio * (float)d2;
            if ((left && lane == win) || lane == winr) { my_free = false; st(match + my_fb, fa); }
          } else {
            int best = 256, second = 256, pos = INT_MAX, bestr = 256, posr = INT_MAX;
            uint32_t fbest = 0, fbestr = 0;
            for (int j = lane; j < nb; j += 64) {
              const uint32_t fb = fB[b0 + j];
              if (ld(match + fb) != -1) continue;
              const int d = hamming(da, load_desc(dB + (size_t)fb * 32));
              if (fb >= (uint32_t)split) {
                if (d < bestr) { bestr = d; posr = j; fbestr = fb; }
              } else if (d < best) { second = best; best = d; pos = j; fbest = fb; }
              else if (d < second) second = d;
            }
            const int m = wave_min(best);
            if (m > g.th) continue;
            const int wpos = wave_min(best == m ? pos : INT_MAX);
            const bool win = best == m && pos == wpos;
            const int d2 = wave_min(win ? second : best);
            bool winr = false, right = false;
            if (rig) {
              const int mr = wave_min(bestr);
              right = mr <= g.th;
              if (right) {
                const int wposr = wave_min(bestr == mr ? posr : INT_MAX);
                winr = bestr == mr && posr == wposr;
              }
            }
            const bool left = (float)m < g.ratio * (float)d2;
            if (left || right) {
              if (left && win) st(match + fbest, fa);
              if (winr) st(match + fbestr, fa);
              __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // the stores are done before the next query's loads
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
        if (oa) oa[2 * v + (b >= split ? 1 : 0)] = b;
        cnt++;
      }
    }
    if (cnt) atomicAdd(&s_nm, cnt);
    __syncthreads();
    if (tid == 0) g.nm[p] = s_nm;
  }
}

}  // namespace

struct orbx_rigbow : orbx::side::pair::PairHandle {};   // scratch: per workgroup the global path's work list and match row

namespace {

using namespace orbx::side;
using namespace orbx::side::pair;

Side to_side(const orbx_rigbow_side* s) {
  return {(const uint8_t*)s->d_kps, s->d_desc, s->d_counts, s->d_fv_node, s->d_fv_ptr, s->d_fv_feat, s->d_fv_n, s->d_valid, s->d_nleft, s->nframes,
          s->capacity};
}

// what both forms check before anything is copied or launched
int check_call(orbx_rigbow* m, const char* who, const orbx_rigbow_side* a, const orbx_rigbow_side* b, const void* pairs, int npairs, int mode,
               const void* b2a, const void* a2b, const void* nm) {
  int rc = check_sides<true>(m, who, a, b, 0, nullptr, pairs && nm, "pairs or nmatches");
  if (rc != ORBX_OK) return rc;
  if (!b2a && !a2b) return fail(m, ORBX_E_INVALID, std::string(who) + "both match arrays are null");
  if ((rc = check_npairs(m, who, npairs)) != ORBX_OK) return rc;
  if (mode != ORBX_RIGBOW_FRAME && mode != ORBX_RIGBOW_KEYFRAMES) return fail(m, ORBX_E_INVALID, std::string(who) + "unknown mode " + std::to_string(mode));
  return check_sizes<true>(m, who, a, b, npairs, 2LL * std::max(a->capacity, b->capacity), "2 * npairs * capacity");
}

}  // namespace

extern "C" {

int orbx_rigbow_create(orbx_rigbow** out, int device) {
  return create_handle(out, device, "orbx_rigbow_create", orbx_rigbow_destroy, [](orbx_rigbow* m) {
    return open_pair(m, "ORBX_RIGBOW_LDS", "ORBX_RIGBOW_WAVE_NODE", (const void*)k_rigbow_pairs<true>);
  });
}

void orbx_rigbow_destroy(orbx_rigbow* m) { destroy_handle(m); }

const char* orbx_rigbow_last_error(const orbx_rigbow* m) { return last_error(m); }

int orbx_rigbow_stack_device(orbx_rigbow* m, const orbx_rigbow_rig* rig, int cap_s, orbx_keypoint* d_kps_s, uint8_t* d_desc_s, int32_t* d_counts_s,
                             int32_t* d_nleft, void* stream) {
  if (!m) return ORBX_E_INVALID;
  const char* who = "orbx_rigbow_stack_device: ";
  if (!rig || !d_kps_s || !d_desc_s || !d_counts_s || !d_nleft) return fail(m, ORBX_E_INVALID, std::string(who) + "null argument");
  if (!rig->d_kps_l || !rig->d_desc_l || !rig->d_counts_l || !rig->d_kps_r || !rig->d_desc_r || !rig->d_counts_r)
    return fail(m, ORBX_E_INVALID, std::string(who) + "null buffer in the rig");
  if (rig->nframes < 1 || rig->cap_l < 1 || rig->cap_r < 1 || cap_s < 1) return fail(m, ORBX_E_INVALID, std::string(who) + "nframes and the capacities must be at least 1");
  if (rig->nframes > 65535) return fail(m, ORBX_E_INVALID, std::string(who) + "more than 65535 frames in one call");
  if ((long long)rig->nframes * std::max(std::max(rig->cap_l, rig->cap_r), cap_s) > (long long)INT_MAX || (long long)cap_s * kKpWords > (long long)INT_MAX)
    return fail(m, ORBX_E_INVALID, std::string(who) + "nframes * capacity exceeds INT_MAX");
  if ((((uintptr_t)rig->d_desc_l | (uintptr_t)rig->d_desc_r | (uintptr_t)d_desc_s) & 15) != 0)
    return fail(m, ORBX_E_INVALID, std::string(who) + "a descriptor buffer is not 16-byte aligned");
  int rc = same_device(m, who, {rig->d_kps_l, rig->d_desc_l, rig->d_counts_l, rig->d_kps_r, rig->d_desc_r, rig->d_counts_r, d_kps_s, d_desc_s, d_counts_s, d_nleft},
                       "the handle");
  if (rc != ORBX_OK) return rc;
  ORBX_SIDE_HIP(m, hipSetDevice(m->device));
  StackArgs g = {(const uint32_t*)rig->d_kps_l, (const uint4*)rig->d_desc_l, rig->d_counts_l, (const uint32_t*)rig->d_kps_r, (const uint4*)rig->d_desc_r,
                 rig->d_counts_r, (uint32_t*)d_kps_s, (uint4*)d_desc_s, d_counts_s, d_nleft, rig->cap_l, rig->cap_r, cap_s};
  const int bx = std::max(1, std::min(64, (cap_s * kKpWords + kStackThreads - 1) / kStackThreads));
  hipStream_t st = stream ? (hipStream_t)stream : m->st;
  if ((rc = wait_previous(m, st)) != ORBX_OK) return rc;
  hipLaunchKernelGGL(k_rigbow_stack, dim3((unsigned)bx, (unsigned)rig->nframes), dim3(kStackThreads), 0, st, g);
  return record_call(m, st);
}

int orbx_rigbow_pairs_device(orbx_rigbow* m, const orbx_rigbow_side* a, const orbx_rigbow_side* b, const int32_t* d_pairs, int npairs, int mode,
                             float nn_ratio, int check_orientation, int32_t* d_match_b2a, int32_t* d_match_a2b, int32_t* d_nmatches, void* stream) {
  if (!m) return ORBX_E_INVALID;
  const char* who = "orbx_rigbow_pairs_device: ";
  int rc = check_call(m, who, a, b, d_pairs, npairs, mode, d_match_b2a, d_match_a2b, d_nmatches);
  if (rc != ORBX_OK) return rc;
  rc = same_device(m, who, {a->d_kps, a->d_desc, a->d_fv_feat, b->d_kps, b->d_desc, b->d_fv_feat, d_pairs, d_match_b2a, d_match_a2b, d_nmatches}, "the handle");
  if (rc != ORBX_OK) return rc;
  ORBX_SIDE_HIP(m, hipSetDevice(m->device));
  const size_t capA = (size_t)a->capacity, capB = (size_t)b->capacity, capW = std::min(capA, capB);
  const size_t lds = 40 * capB + 8 * capW;
  const bool in_lds = lds <= (size_t)m->lds_limit && capA <= (size_t)kPackedCap && capB <= (size_t)kPackedCap;
  Args g;
  g.a = to_side(a); g.b = to_side(b);
  g.pairs = d_pairs; g.b2a = d_match_b2a; g.a2b = d_match_a2b; g.nm = d_nmatches;
  g.npairs = npairs; g.th = mode == ORBX_RIGBOW_KEYFRAMES ? 49 : 50; g.kf = mode == ORBX_RIGBOW_KEYFRAMES; g.check_ori = check_orientation != 0;
  g.wave_node = m->wave_node; g.ratio = nn_ratio;
  return launch(m, in_lds, lds, (((capW * 16 + 15) & ~(size_t)15) + capB * 4 + 255) & ~(size_t)255, std::min(npairs, kMaxBlocks), kThreads, g,
                k_rigbow_pairs<true>, k_rigbow_pairs<false>, stream);
}

int orbx_rigbow_pairs(orbx_rigbow* m, const orbx_rigbow_side* a, const orbx_rigbow_side* b, const int32_t* pairs, int npairs, int mode, float nn_ratio,
                      int check_orientation, int32_t* match_b2a, int32_t* match_a2b, int32_t* nmatches) {
  if (!m) return ORBX_E_INVALID;
  const char* who = "orbx_rigbow_pairs: ";
  int rc = check_call(m, who, a, b, pairs, npairs, mode, match_b2a, match_a2b, nmatches);
  if (rc != ORBX_OK) return rc;
  const auto arrays = side_arrays<true, orbx_rigbow_side>({{offsetof(orbx_rigbow_side, d_valid), 0, 1, true}, {offsetof(orbx_rigbow_side, d_nleft), 4, 0, true}});
  Stager io;
  const StagedSides off = stage_sides(io, a, b, arrays);
  const size_t o_pairs = io.in(pairs, (size_t)npairs * 8);
  const size_t o_b2a = io.out(match_b2a, (size_t)npairs * b->capacity * 4), o_a2b = io.out(match_a2b, (size_t)npairs * a->capacity * 8),
               o_nm = io.out(nmatches, (size_t)npairs * 4);
  if ((rc = upload(m, io)) != ORBX_OK) return rc;
  uint8_t* d = m->io.p;
  orbx_rigbow_side ds[2];
  device_sides(d, off, a, b, arrays, ds);
  rc = orbx_rigbow_pairs_device(m, &ds[0], &ds[1], (const int32_t*)(d + o_pairs), npairs, mode, nn_ratio, check_orientation, (int32_t*)(d + o_b2a),
                                (int32_t*)(d + o_a2b), (int32_t*)(d + o_nm), m->st);
  if (rc != ORBX_OK) return rc;
  return download(m, io);
}

}  // extern "C"
