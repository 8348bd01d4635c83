// The batched SearchForInitialization (include/orbx_initmatch.h): ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:648-763) for P
// (frame, frame) pairs on the keypoints, descriptors and counts a batch extraction left in HBM.
//
// k_init_pairs<LDS>: one workgroup of 8 waves per pair (a grid of at most kMaxBlocks workgroups walks the pairs).
//   phase A, all waves   validate; collect F2's level-0 keypoints as keys (cell << 16 | index), sort them (bitonic, keys are unique: the
//                        order is the frame grid's: cells x-major, then y, then ascending index), the cells' starts by binary search;
//                        a thread per level-0 query counts its window's candidates, a scan turns the counts into offsets.
//                        Then, for a chunk of queries whose lists fit the candidate room: a thread per query writes its list in reference
//                        order (a grid column of a window is one contiguous run of sorted keys), a thread per candidate computes its Hamming
//                        distance; a candidate is one 32-bit word: index in the low, distance in the high 16 bits.
//   phase B, wave 0      the chain over the chunk's queries in index order: lane j holds candidate j (+ 64 per trip), gathers
//                        vMatchedDistance[i2], masks, and the best / first position / second come from three DPP min-reductions; one lane
//                        applies accept, steal and update.  No descriptor and no keypoint is read here.
//                        A and B repeat per chunk: the distances do not depend on the chain, so where the chunks are cut changes nothing.
//   phase C, all waves   the rotation histogram from what every query held when it was accepted (never undone), ComputeThreeMaxima on one
//                        lane, then a thread per query drops the losers and writes matches12, matches21, prev_xy and the count.
// LDS path: the two descriptor sets (16-byte LDS-DMA loads), the grid, the offsets, the chain's state and the candidate room in LDS.
// Global path (capacities that need more LDS than the handle's limit): the descriptors where they lie, everything else in the workgroup's
// slice of the handle's scratch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../side/orbx_handle.h"
#include "../../../include/orbx_initmatch.h"

namespace {

constexpr int kThreads = 512;             // 8 waves
constexpr int kLdsMax = 152 * 1024;       // dynamic LDS of one workgroup (160 KiB per CU, the static part is below 4 KiB)
constexpr int kMaxBlocks = 1024;          // workgroups of one launch on the LDS path
constexpr int kGlobalBlocks = 256;        // ... on the global path: each owns one slice of the scratch
constexpr int kGlobalRoom = 64 * 1024;    // candidates of one chunk on the global path (at least capB)
constexpr int kMaxCap = 32768;            // a key holds a 15-bit index, a candidate a 16-bit one
constexpr int kCols = 64, kRows = 48, kCells = kCols * kRows;
constexpr int kThLow = 50;

struct Side { const uint8_t* kps; const uint8_t* desc; const int32_t* counts; int nframes, cap; };

struct Args {
  Side a, b;
  const int32_t* pairs;
  float* prev; int32_t* m12; int32_t* m21; int32_t* nm;
  uint8_t* scratch; size_t scratch_stride;
  int npairs, p2, room, check_ori;
  float minX, minY, invW, invH, r, ratio;
};

// one pair's arrays, as offsets in the LDS block resp. the scratch slice (16-byte aligned)
struct Lay { size_t dA, dB, keys, sxy, cstart, offs, mdist, holder, m12, acc, cand, fixed; };
__host__ __device__ inline Lay layout(int capA, int capB, int p2, bool lds) {
  Lay l;
  size_t o = 0;
  auto add = [&](size_t bytes) { const size_t at = o; o = (o + bytes + 15) & ~(size_t)15; return at; };
  l.dA = add(lds ? (size_t)capA * 32 : 0);
  l.dB = add(lds ? (size_t)capB * 32 : 0);
  l.keys = add((size_t)p2 * 4);             // sorted (cell << 16 | index) of F2's level-0 keypoints
  l.sxy = add((size_t)capB * 8);            // their positions, in the same order
  l.cstart = add((size_t)(kCells + 1) * 2); // first sorted position of every cell
  l.offs = add((size_t)(capA + 1) * 4);     // first candidate of every query (exclusive scan of the counts)
  l.mdist = add((size_t)capB * 4);          // vMatchedDistance
  l.holder = add((size_t)capB * 4);         // vnMatches21 during the chain
  l.m12 = add((size_t)capA * 4);            // vnMatches12
  l.acc = add((size_t)capA * 4);            // the F2 feature a query was accepted with: never undone
  l.cand = o;
  l.fixed = o;
  return l;
}

struct D8 { uint32_t w[8]; };
__device__ __forceinline__ D8 load_desc(const uint8_t* p) {
  const uint4 x = ((const uint4*)p)[0], y = ((const uint4*)p)[1];
  D8 d;
  d.w[0] = x.x; d.w[1] = x.y; d.w[2] = x.z; d.w[3] = x.w; d.w[4] = y.x; d.w[5] = y.y; d.w[6] = y.z; d.w[7] = y.w;
  return d;
}
__device__ __forceinline__ int hamming(const D8& a, const D8& b) {
  int s = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) s += __popc(a.w[k] ^ b.w[k]);
  return s;
}

// the minimum over the 64 lanes (all active), wave-uniform: four DPP steps leave each row of 16 lanes with its minimum, the four rows meet
// through readlane
__device__ __forceinline__ int wave_min(int v) {
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, false));    // quad_perm [1, 0, 3, 2]
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, false));    // quad_perm [2, 3, 0, 1]
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xF, 0xF, false));   // row_half_mirror
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xF, 0xF, false));   // row_mirror
  return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
             min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

// the chain's state is written by one lane and read by the wave's other lanes in the next step
__device__ __forceinline__ int ld_state(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void st_state(int32_t* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// the rotation histogram's bin (src/ORBmatcher.cc:718-725), -1 when it falls outside the 30 bins (then the match is never removed)
__device__ __forceinline__ int rot_bin(float angle_a, float angle_b) {
  float rot = angle_a - angle_b;
  if (rot < 0.0f) rot += 360.0f;
  const float r = roundf(rot * (1.0f / 30));
  if (!(r >= 0.0f && r <= 30.0f)) return -1;
  const int bin = (int)r;
  return bin == 30 ? 0 : bin;
}
__device__ __forceinline__ float kp_f(const uint8_t* kps, size_t i, size_t field) { return *(const float*)(kps + i * sizeof(orbx_keypoint) + field); }
__device__ __forceinline__ int kp_octave(const uint8_t* kps, size_t i) { return *(const int32_t*)(kps + i * sizeof(orbx_keypoint) + offsetof(orbx_keypoint, octave)); }
constexpr size_t kX = offsetof(orbx_keypoint, x), kY = offsetof(orbx_keypoint, y), kAngle = offsetof(orbx_keypoint, angle);

// n16 16-byte pieces from src to the LDS block at dst: piece i lands at dst + 16 i (lane-linear inside a wave, as the LDS-DMA load writes)
__device__ __forceinline__ void stage_dma(uint8_t* dst, const uint8_t* src, int n16) {
  for (int i0 = 0; i0 < n16; i0 += kThreads) {
    const int i = i0 + (int)threadIdx.x;
    uint8_t* d = dst + (size_t)(i0 + ((int)threadIdx.x & ~63)) * 16;   // wave-uniform; the hardware adds lane * 16
    if (i < n16)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + (size_t)i * 16),
                                       (__attribute__((address_space(3))) void*)d, 16, 0, 0);
  }
}

// Frame::GetFeaturesInArea(x, y, r, 0, 0) over the sorted keys: emit(index) for every candidate, in the reference's order
template <class F>
__device__ __forceinline__ void walk(const Args& g, float x, float y, const uint16_t* cstart, const uint32_t* keys, const float2* sxy, F emit) {
  const float r = g.r;
  const int x0 = max(0, (int)floorf((x - g.minX - r) * g.invW));
  if (x0 >= kCols) return;
  const int x1 = min(kCols - 1, (int)ceilf((x - g.minX + r) * g.invW));
  if (x1 < 0) return;
  const int y0 = max(0, (int)floorf((y - g.minY - r) * g.invH));
  if (y0 >= kRows) return;
  const int y1 = min(kRows - 1, (int)ceilf((y - g.minY + r) * g.invH));
  if (y1 < 0) return;
  if (y1 < y0) return;                     // an empty range of rows (the reference's inner loop does not run)
  for (int ix = x0; ix <= x1; ix++) {      // the cells (ix, y0 .. y1) are neighbours in the sorted keys
    const int j1 = cstart[ix * kRows + y1 + 1];
    for (int j = cstart[ix * kRows + y0]; j < j1; j++) {
      const float2 p = sxy[j];
      if (fabsf(p.x - x) < r && fabsf(p.y - y) < r) emit((int)(keys[j] & 0xFFFFu));
    }
  }
}

template <bool LDS>
__global__ __launch_bounds__(kThreads) void k_init_pairs(Args g) {
  extern __shared__ __align__(16) uint8_t smem[];
  __shared__ int s_cnt, s_nm;
  __shared__ int s_scan[kThreads];
  __shared__ int s_hist[32];
  __shared__ int s_ind[3];
  const int tid = threadIdx.x, lane = tid & 63;
  const int capA = g.a.cap, capB = g.b.cap;
  const Lay L = layout(capA, capB, g.p2, LDS);
  uint8_t* const base = LDS ? smem : g.scratch + (size_t)blockIdx.x * g.scratch_stride;
  uint32_t* const keys = (uint32_t*)(base + L.keys);
  float2* const sxy = (float2*)(base + L.sxy);
  uint16_t* const cstart = (uint16_t*)(base + L.cstart);
  int32_t* const offs = (int32_t*)(base + L.offs);
  int32_t* const mdist = (int32_t*)(base + L.mdist);
  int32_t* const holder = (int32_t*)(base + L.holder);
  int32_t* const m12 = (int32_t*)(base + L.m12);
  int32_t* const acc = (int32_t*)(base + L.acc);
  uint32_t* const cand = (uint32_t*)(base + L.cand);

  for (int p = blockIdx.x; p < g.npairs; p += gridDim.x) {
    __syncthreads();                       // the previous pair's shared state has been read
    const int ia = g.pairs[2 * p], ib = g.pairs[2 * p + 1];
    int32_t* const o12 = g.m12 + (size_t)p * capA;
    int32_t* const o21 = g.m21 ? g.m21 + (size_t)p * capB : nullptr;
    bool ok = ia >= 0 && ia < g.a.nframes && ib >= 0 && ib < g.b.nframes;
    int nA = 0, nB = 0;
    if (ok) {
      nA = g.a.counts[2 * ia]; nB = g.b.counts[2 * ib];
      ok = nA >= 0 && nA <= capA && nB >= 0 && nB <= capB;
    }
    if (!ok) {                             // uniform over the workgroup
      for (int i = tid; i < capA; i += kThreads) o12[i] = -1;
      if (o21) for (int i = tid; i < capB; i += kThreads) o21[i] = -1;
      if (tid == 0) g.nm[p] = -1;
      continue;
    }
    const size_t oA = (size_t)ia * capA, oB = (size_t)ib * capB;
    const uint8_t* const kA = g.a.kps + oA * sizeof(orbx_keypoint);
    const uint8_t* const kB = g.b.kps + oB * sizeof(orbx_keypoint);
    const uint8_t* const dA = LDS ? base + L.dA : g.a.desc + oA * 32;
    const uint8_t* const dB = LDS ? base + L.dB : g.b.desc + oB * 32;
    float* const prev = g.prev ? g.prev + ((size_t)p * capA) * 2 : nullptr;

    // ---- phase A: F2's grid
    if (tid == 0) { s_cnt = 0; s_nm = 0; }
    if (tid < 32) s_hist[tid] = 0;
    if (LDS) {
      stage_dma(base + L.dA, g.a.desc + oA * 32, nA * 2);
      stage_dma(base + L.dB, g.b.desc + oB * 32, nB * 2);
    }
    for (int i = tid; i < nB; i += kThreads) { mdist[i] = INT_MAX; holder[i] = -1; }
    for (int i = tid; i < nA; i += kThreads) { m12[i] = -1; acc[i] = -1; }
    __syncthreads();                       // s_cnt = 0 before anyone adds to it
    for (int i = tid; i < nB; i += kThreads) {
      if (kp_octave(kB, i) != 0) continue;
      const float fx = roundf((kp_f(kB, i, kX) - g.minX) * g.invW), fy = roundf((kp_f(kB, i, kY) - g.minY) * g.invH);
      if (!(fx >= 0.0f && fx < (float)kCols && fy >= 0.0f && fy < (float)kRows)) continue;   // outside the grid (or NaN): in no cell
      const int k = atomicAdd(&s_cnt, 1);  // k < nB <= capB <= p2
      keys[k] = (uint32_t)((int)fx * kRows + (int)fy) << 16 | (uint32_t)i;
    }
    __syncthreads();
    const int n0 = s_cnt;                  // F2's level-0 keypoints inside the grid
    int n2 = 2;
    while (n2 < n0) n2 <<= 1;              // n2 <= p2
    for (int i = n0 + tid; i < n2; i += kThreads) keys[i] = 0xFFFFFFFFu;
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = tid; t < (n2 >> 1); t += kThreads) {
          const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
          const uint32_t a = keys[i], b = keys[l];
          if ((a > b) == ((i & k) == 0)) { keys[i] = b; keys[l] = a; }
        }
        __syncthreads();
      }
    for (int j = tid; j < n0; j += kThreads) {
      const size_t i = keys[j] & 0xFFFFu;
      sxy[j] = make_float2(kp_f(kB, i, kX), kp_f(kB, i, kY));
    }
    for (int c = tid; c <= kCells; c += kThreads) {
      const uint32_t want = (uint32_t)c << 16;
      int lo = 0, hi = n0;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < want) lo = mid + 1; else hi = mid;
      }
      cstart[c] = (uint16_t)lo;            // <= 32768
    }
    __syncthreads();

    // ---- phase A: every query's candidate count, then the offsets
    for (int q = tid; q <= nA; q += kThreads) {
      int c = 0;
      if (q < nA && kp_octave(kA, q) == 0) {
        const float cx = prev ? prev[2 * q] : kp_f(kA, q, kX), cy = prev ? prev[2 * q + 1] : kp_f(kA, q, kY);
        walk(g, cx, cy, cstart, keys, sxy, [&](int) { c++; });
      }
      offs[q] = c;
    }
    __syncthreads();
    {
      const int n = nA + 1, per = (n + kThreads - 1) / kThreads;
      const int lo = min(n, tid * per), hi = min(n, lo + per);
      int s = 0;
      for (int i = lo; i < hi; i++) s += offs[i];
      s_scan[tid] = s;
      __syncthreads();
      for (int d = 1; d < kThreads; d <<= 1) {
        const int v = tid >= d ? s_scan[tid - d] : 0;
        __syncthreads();
        s_scan[tid] += v;
        __syncthreads();
      }
      int run = s_scan[tid] - s;
      for (int i = lo; i < hi; i++) { const int c = offs[i]; offs[i] = run; run += c; }
    }
    if (LDS) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the LDS-DMA loads have landed
    __syncthreads();

    // ---- chunks of queries whose candidates fit the room: lists and distances (all waves), then the chain (wave 0)
    for (int q0 = 0; q0 < nA;) {
      const int e0 = offs[q0];
      int q1;
      {                                    // the largest q1 with offs[q1] - e0 <= room; one query's list (<= capB <= room) always fits
        int lo = q0 + 1, hi = nA;
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if (offs[mid] - e0 <= g.room) lo = mid; else hi = mid - 1;
        }
        q1 = lo;
      }
      const int tot = min(offs[q1] - e0, g.room);
      for (int q = q0 + tid; q < q1; q += kThreads) {
        int k = offs[q] - e0;
        const int kend = offs[q + 1] - e0;
        if (kend > k) {
          const float cx = prev ? prev[2 * q] : kp_f(kA, q, kX), cy = prev ? prev[2 * q + 1] : kp_f(kA, q, kY);
          walk(g, cx, cy, cstart, keys, sxy, [&](int i2) { if (k < kend && k < tot) cand[k] = (uint32_t)i2; k++; });
        }
      }
      __syncthreads();
      for (int e = tid; e < tot; e += kThreads) {
        int lo = q0, hi = q1 - 1;          // the query of candidate e: the largest q with offs[q] <= e0 + e
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if (offs[mid] - e0 <= e) lo = mid; else hi = mid - 1;
        }
        const uint32_t i2 = cand[e] & 0xFFFFu;
        const int d = hamming(load_desc(dA + (size_t)lo * 32), load_desc(dB + (size_t)i2 * 32));
        cand[e] = i2 | (uint32_t)d << 16;
      }
      __syncthreads();

#ifndef ORBX_INITMATCH_NO_CHAIN           // (a timing build without phase B: tools/initmatch_times.py; its results are not the specification's)
      if (tid < 64) {                      // ---- phase B
        for (int c0 = q0; c0 < q1; c0 += 64) {
          const int cn = min(64, q1 - c0);
          int l_b = 0, l_n = 0;
          if (lane < cn) { l_b = offs[c0 + lane] - e0; l_n = offs[c0 + lane + 1] - e0 - l_b; }
          for (int i = 0; i < cn; i++) {
            const int n = __builtin_amdgcn_readlane(l_n, i);
            if (n <= 0) continue;
            const int b0 = __builtin_amdgcn_readlane(l_b, i);
            int best = INT_MAX, second = INT_MAX, pos = INT_MAX, ibest = 0;
            for (int j = lane; j < n; j += 64) {
              const uint32_t e = cand[b0 + j];
              const int i2 = (int)(e & 0xFFFFu), d = (int)(e >> 16);
              if (ld_state(mdist + i2) <= d) continue;
              if (d < best) { second = best; best = d; pos = j; ibest = i2; }
              else if (d < second) second = d;
            }
            const int m = wave_min(best);
            if (m > kThLow) continue;
            const int wpos = wave_min(best == m ? pos : INT_MAX);
            const bool win = best == m && pos == wpos;
            const int d2 = wave_min(win ? second : best);
            if ((float)m < (float)d2 * g.ratio) {
              if (win) {
                const int q = c0 + i;
                const int was = ld_state(holder + ibest);
                if (was >= 0) st_state(m12 + was, -1);
                st_state(m12 + q, ibest);
                st_state(acc + q, ibest);
                st_state(holder + ibest, q);
                st_state(mdist + ibest, m);
              }
              __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // the stores are done before the next query's loads
            }
          }
        }
      }
#endif
      __syncthreads();
      q0 = q1;
    }

    // ---- phase C: the rotation filter and the outputs
    int i1 = -1, i2 = -1, i3 = -1;
    if (g.check_ori) {
      for (int q = tid; q < nA; q += kThreads) {
        const int v = acc[q];
        if (v >= 0) {
          const int bin = rot_bin(kp_f(kA, q, kAngle), kp_f(kB, v, kAngle));
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
    if (o21) for (int i = tid; i < capB; i += kThreads) o21[i] = -1;
    __syncthreads();                       // before the matches are scattered into the row
    int cnt = 0;
    for (int q = tid; q < capA; q += kThreads) {
      int v = -1;
      if (q < nA) {
        v = m12[q];
        if (v >= 0 && g.check_ori) {       // a standing match is the one the query was accepted with: its bin is the recorded one
          const int bin = rot_bin(kp_f(kA, q, kAngle), kp_f(kB, v, kAngle));
          if (bin >= 0 && bin != i1 && bin != i2 && bin != i3) v = -1;
        }
        if (v < 0 || v >= nB) v = -1;
      }
      o12[q] = v;
      if (v >= 0) {
        if (o21) o21[v] = q;
        if (prev) { prev[2 * q] = kp_f(kB, v, kX); prev[2 * q + 1] = kp_f(kB, v, kY); }
        cnt++;
      }
    }
    if (cnt) atomicAdd(&s_nm, cnt);
    __syncthreads();
    if (tid == 0) g.nm[p] = s_nm;
  }
}

}  // namespace

struct orbx_initmatch : orbx::side::Handle {   // scratch: per workgroup the global path's arrays
  int lds_limit = kLdsMax;                     // ORBX_INITMATCH_LDS at create
  std::vector<uint8_t> h_io;                   // the host form's results before they are handed out
};

namespace {

using namespace orbx::side;

struct HostLayout {                            // offsets in one block, 256-byte aligned
  size_t size = 0;
  size_t add(size_t bytes) { const size_t o = size; size = (size + bytes + 255) & ~(size_t)255; return o; }
};

const char* side_problem(const orbx_initmatch_side* s) {
  if (!s) return "null side";
  if (s->nframes < 1 || s->capacity < 1) return "nframes and capacity must be at least 1";
  if (s->capacity > kMaxCap) return "capacity above 32768";
  if (!s->d_kps || !s->d_desc || !s->d_counts) return "null buffer in a side";
  return nullptr;
}

// what both forms check before anything is copied or launched
int check_call(orbx_initmatch* m, const char* who, const orbx_initmatch_side* a, const orbx_initmatch_side* b, const void* pairs, int npairs,
               const float* bounds, int window, const void* m12, const void* nm) {
  for (const orbx_initmatch_side* s : {a, b})
    if (const char* e = side_problem(s)) return fail(m, ORBX_E_INVALID, std::string(who) + e);
  if (!pairs || !m12 || !nm || !bounds) return fail(m, ORBX_E_INVALID, std::string(who) + "null pairs, bounds, matches12 or nmatches");
  if (npairs < 1) return fail(m, ORBX_E_INVALID, std::string(who) + "npairs = " + std::to_string(npairs) + " (at least 1)");
  if (window < 0) return fail(m, ORBX_E_INVALID, std::string(who) + "window_size = " + std::to_string(window) + " (at least 0)");
  if (!(bounds[2] > bounds[0]) || !(bounds[3] > bounds[1])) return fail(m, ORBX_E_INVALID, std::string(who) + "bounds: max must be above min");
  if ((long long)npairs * std::max(a->capacity, b->capacity) * 2 > (long long)INT_MAX || (long long)a->nframes * a->capacity > (long long)INT_MAX ||
      (long long)b->nframes * b->capacity > (long long)INT_MAX)
    return fail(m, ORBX_E_INVALID, std::string(who) + "npairs * capacity or nframes * capacity exceeds INT_MAX");
  return ORBX_OK;
}

}  // namespace

extern "C" {

int orbx_initmatch_create(orbx_initmatch** out, int device) {
  if (out) *out = nullptr;
  if (!out) return create_fail(ORBX_E_INVALID, "orbx_initmatch_create", "null argument");
  if (device < 0) return create_fail(ORBX_E_INVALID, "orbx_initmatch_create", "device must be >= 0");
  orbx_initmatch* m = new orbx_initmatch();
  if (const char* e = std::getenv("ORBX_INITMATCH_LDS")) m->lds_limit = std::max(0, std::min(kLdsMax, std::atoi(e)));
  const char* e = open_handle(m, device);
  if (!e && hipFuncSetAttribute((const void*)k_init_pairs<true>, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax) != hipSuccess) {
    (void)hipGetLastError();
    e = "the kernel's LDS size was refused";
  }
  if (e) { orbx_initmatch_destroy(m); return create_fail(ORBX_E_DEVICE, "orbx_initmatch_create", e); }
  *out = m;
  return ORBX_OK;
}

void orbx_initmatch_destroy(orbx_initmatch* m) {
  if (!m) return;
  close_handle(m);
  delete m;
}

const char* orbx_initmatch_last_error(const orbx_initmatch* m) { return last_error(m); }

int orbx_initmatch_pairs_device(orbx_initmatch* m, const orbx_initmatch_side* a, const orbx_initmatch_side* b, const int32_t* d_pairs, int npairs,
                                const float bounds[4], int window_size, float nn_ratio, int check_orientation, float* d_prev_xy,
                                int32_t* d_matches12, int32_t* d_matches21, int32_t* d_nmatches, void* stream) {
  if (!m) return ORBX_E_INVALID;
  const char* who = "orbx_initmatch_pairs_device: ";
  int rc = check_call(m, who, a, b, d_pairs, npairs, bounds, window_size, d_matches12, d_nmatches);
  if (rc != ORBX_OK) return rc;
  for (const void* p : {(const void*)a->d_kps, (const void*)a->d_desc, (const void*)a->d_counts, (const void*)b->d_kps, (const void*)b->d_desc,
                        (const void*)b->d_counts, (const void*)d_pairs, (const void*)d_prev_xy, (const void*)d_matches12, (const void*)d_matches21,
                        (const void*)d_nmatches}) {
    const int pd = pointer_device(p);
    if (pd >= 0 && pd != m->device)
      return fail(m, ORBX_E_INVALID, std::string(who) + "a buffer lives on device " + std::to_string(pd) + ", the handle on device " + std::to_string(m->device));
  }
  ORBX_SIDE_HIP(m, hipSetDevice(m->device));
  const int capA = a->capacity, capB = b->capacity;
  int p2 = 2;
  while (p2 < capB) p2 <<= 1;
  // the LDS path needs its arrays and room for one query's longest list (capB candidates); what is left of the limit is candidate room
  const size_t fixed = layout(capA, capB, p2, true).fixed;
  const size_t lds_limit = (size_t)m->lds_limit & ~(size_t)15;
  const bool in_lds = fixed + 4 * (size_t)capB <= lds_limit;
  Args g;
  g.a = {(const uint8_t*)a->d_kps, a->d_desc, a->d_counts, a->nframes, capA};
  g.b = {(const uint8_t*)b->d_kps, b->d_desc, b->d_counts, b->nframes, capB};
  g.pairs = d_pairs; g.prev = d_prev_xy; g.m12 = d_matches12; g.m21 = d_matches21; g.nm = d_nmatches;
  g.scratch = nullptr; g.scratch_stride = 0;
  g.npairs = npairs; g.p2 = p2; g.check_ori = check_orientation != 0;
  g.minX = bounds[0]; g.minY = bounds[1];
  g.invW = (float)kCols / (bounds[2] - bounds[0]); g.invH = (float)kRows / (bounds[3] - bounds[1]);
  g.r = (float)window_size; g.ratio = nn_ratio;
  size_t lds = 0;
  int blocks;
  if (in_lds) {
    lds = lds_limit;
    g.room = (int)((lds - fixed) / 4);
    blocks = std::min(npairs, kMaxBlocks);
  } else {
    g.room = std::max(capB, kGlobalRoom);
    blocks = std::min(npairs, kGlobalBlocks);
    g.scratch_stride = (layout(capA, capB, p2, false).fixed + 4 * (size_t)g.room + 255) & ~(size_t)255;
    if ((rc = grow(m, &m->scratch, g.scratch_stride * blocks)) != ORBX_OK) return rc;
    g.scratch = m->scratch.p;
  }
  hipStream_t st = stream ? (hipStream_t)stream : m->st;
  if ((rc = wait_previous(m, st)) != ORBX_OK) return rc;
  if (in_lds) hipLaunchKernelGGL(k_init_pairs<true>, dim3((unsigned)blocks), dim3(kThreads), lds, st, g);
  else hipLaunchKernelGGL(k_init_pairs<false>, dim3((unsigned)blocks), dim3(kThreads), 0, st, g);
  return record_call(m, st);
}

int orbx_initmatch_pairs(orbx_initmatch* m, const orbx_initmatch_side* a, const orbx_initmatch_side* b, const int32_t* pairs, int npairs,
                         const float bounds[4], int window_size, float nn_ratio, int check_orientation, float* prev_xy, int32_t* matches12,
                         int32_t* matches21, int32_t* nmatches) {
  if (!m) return ORBX_E_INVALID;
  const char* who = "orbx_initmatch_pairs: ";
  int rc = check_call(m, who, a, b, pairs, npairs, bounds, window_size, matches12, nmatches);
  if (rc != ORBX_OK) return rc;
  const bool same = a == b || std::memcmp(a, b, sizeof(*a)) == 0;   // one batch on both sides is staged once
  HostLayout io;
  struct Off { size_t kps, desc, counts; } off[2];
  const orbx_initmatch_side* sides[2] = {a, b};
  for (int s = 0; s < (same ? 1 : 2); s++) {
    const size_t nf = (size_t)sides[s]->nframes, nk = nf * sides[s]->capacity;
    off[s] = {io.add(nk * sizeof(orbx_keypoint)), io.add(nk * 32), io.add(nf * 8)};
  }
  if (same) off[1] = off[0];
  const size_t o_pairs = io.add((size_t)npairs * 8);
  const size_t n12 = (size_t)npairs * a->capacity * 4, n21 = (size_t)npairs * b->capacity * 4, nprev = prev_xy ? n12 * 2 : 0;
  const size_t o_out = io.size;                // the results, read back in one copy
  const size_t o_prev = io.add(nprev), o_12 = io.add(n12), o_21 = io.add(n21), o_nm = io.add((size_t)npairs * 4);
  ORBX_SIDE_HIP(m, hipSetDevice(m->device));
  if ((rc = grow(m, &m->io, io.size)) != ORBX_OK) return rc;
  if (m->h_io.size() < io.size - o_out) m->h_io.resize(io.size - o_out);
  uint8_t* d = m->io.p;
  hipStream_t st = m->st;
  if ((rc = wait_previous(m, st)) != ORBX_OK) return rc;
  orbx_initmatch_side ds[2];
  for (int s = 0; s < 2; s++) {
    const orbx_initmatch_side* h = sides[s];
    const Off& o = off[s];
    const size_t nf = (size_t)h->nframes, nk = nf * h->capacity;
    if (s == 0 || !same) {
      ORBX_SIDE_HIP(m, hipMemcpyAsync(d + o.kps, h->d_kps, nk * sizeof(orbx_keypoint), hipMemcpyHostToDevice, st));
      ORBX_SIDE_HIP(m, hipMemcpyAsync(d + o.desc, h->d_desc, nk * 32, hipMemcpyHostToDevice, st));
      ORBX_SIDE_HIP(m, hipMemcpyAsync(d + o.counts, h->d_counts, nf * 8, hipMemcpyHostToDevice, st));
    }
    ds[s] = {(const orbx_keypoint*)(d + o.kps), d + o.desc, (const int32_t*)(d + o.counts), h->nframes, h->capacity};
  }
  ORBX_SIDE_HIP(m, hipMemcpyAsync(d + o_pairs, pairs, (size_t)npairs * 8, hipMemcpyHostToDevice, st));
  if (prev_xy) ORBX_SIDE_HIP(m, hipMemcpyAsync(d + o_prev, prev_xy, nprev, hipMemcpyHostToDevice, st));
  rc = orbx_initmatch_pairs_device(m, &ds[0], &ds[1], (const int32_t*)(d + o_pairs), npairs, bounds, window_size, nn_ratio, check_orientation,
                                   prev_xy ? (float*)(d + o_prev) : nullptr, (int32_t*)(d + o_12), (int32_t*)(d + o_21), (int32_t*)(d + o_nm), st);
  if (rc != ORBX_OK) return rc;
  uint8_t* h = m->h_io.data();
  ORBX_SIDE_HIP(m, hipMemcpyAsync(h, d + o_out, io.size - o_out, hipMemcpyDeviceToHost, st));
  if ((rc = finish_host(m)) != ORBX_OK) return rc;
  if (prev_xy) std::memcpy(prev_xy, h + o_prev - o_out, nprev);
  std::memcpy(matches12, h + o_12 - o_out, n12);
  if (matches21) std::memcpy(matches21, h + o_21 - o_out, n21);
  std::memcpy(nmatches, h + o_nm - o_out, (size_t)npairs * 4);
  return ORBX_OK;
}

}  // extern "C"
