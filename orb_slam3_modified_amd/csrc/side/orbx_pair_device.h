// The device helpers the side libraries' matching kernels share: descriptors and Hamming distances, the wave minimum, the 32-bit top-2
// keys, a chain's relaxed loads and stores, the rotation bin, the keypoint field reader, the LDS-DMA staging, a frame grid's record, a work
// list's pop, the workgroup scan and, for k_tri_pairs and k_init_pairs, the FeatureVector node intersection and ComputeThreeMaxima.
// Every source below csrc/ that includes this file is a user; the frame grid and the window of the four chained projection matchers
// are built on it in orbx_window_device.h.  Device code only; it sits below csrc/, outside kernels_hash().  A kernel's file imports the
// names with `using namespace orbx::side::dev;` inside its anonymous namespace.
// k_match_pairs and k_rigbow_pairs keep their own text of both: as one core their one-node trip loop measured 1.3 to 2.4 % slower
// (profiles/bowpair_core_refactor.txt).  The trip loop's three-reduction merge stays written out where it is used.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "../../../include/orbx.h"

namespace orbx {
namespace side {
namespace dev {

struct D8 { uint32_t w[8]; };

// a sorted position's record in a frame grid (k_fuse_search, orbx_window_device.h): what a window test reads of its keypoint
struct __align__(16) Rec { float x, y; int32_t octave; float ur; };

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

// The two smallest (distance, train index) keys of a sequential scan, as csrc/orbx_matcher.hip's k_knn2_partial keeps them: one 32-bit key
// distance (0 .. 256) << 22 | index (< 2^22), so that equal distances order by index and the update is three min / max instructions.
constexpr uint32_t kNoKey32 = 0xffffffffu;
constexpr int kKeyIndexBits = 22;
struct Top2x32 { uint32_t k1, k2; };
__device__ __forceinline__ Top2x32 top2_push(Top2x32 t, uint32_t dist, uint32_t index) {
  const uint32_t key = (dist << kKeyIndexBits) | index;
  const uint32_t hi = max(t.k1, key);
  t.k1 = min(t.k1, key);
  t.k2 = min(t.k2, hi);
  return t;
}
__device__ __forceinline__ int key_index(uint32_t k) { return k == kNoKey32 ? -1 : (int)(k & ((1u << kKeyIndexBits) - 1u)); }
__device__ __forceinline__ int key_dist(uint32_t k) { return k == kNoKey32 ? 256 : (int)(k >> kKeyIndexBits); }

// the minimum over the 64 lanes (all active), wave-uniform: four DPP steps leave each row of 16 lanes with its minimum (lane <-> lane ^ 1,
// lane ^ 2, mirror of the half row, mirror of the row), the four rows meet through readlane
__device__ __forceinline__ int wave_min(int v) {
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, false));    // quad_perm [1, 0, 3, 2]
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, false));    // quad_perm [2, 3, 0, 1]
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xF, 0xF, false));   // row_half_mirror
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xF, 0xF, false));   // row_mirror
  return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
             min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

// a chain's state is written by one lane and read by the wave's other lanes in the next step of the same chain
__device__ __forceinline__ int ld(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void st(int32_t* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// the rotation histogram's bin of a match (src/ORBmatcher.cc:302-311, :718-725), -1 when it falls outside the 30 bins (then the match is
// never removed)
__device__ __forceinline__ int rot_bin(float angle_a, float angle_b) {
  float rot = angle_a - angle_b;
  if (rot < 0.0f) rot += 360.0f;
  const float r = roundf(rot * (1.0f / 30));
  if (!(r >= 0.0f && r <= 30.0f)) return -1;
  const int bin = (int)r;
  return bin == 30 ? 0 : bin;
}

// ComputeThreeMaxima (src/ORBmatcher.cc:2012-2053) on one lane: the three fullest of hist's 30 bins into ind[0 .. 2], -1 as there
__device__ __forceinline__ void three_maxima(const int* hist, int* ind) {
  int ind1 = -1, ind2 = -1, ind3 = -1, max1 = 0, max2 = 0, max3 = 0;
  int h[30];                               // all bins first: one wait on the one lane the workgroup waits for
#pragma unroll
  for (int i = 0; i < 30; i++) h[i] = hist[i];
#pragma unroll
  for (int i = 0; i < 30; i++) {
    const int s = h[i];
    if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
    else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
    else if (s > max3) { max3 = s; ind3 = i; }
  }
  if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
  else if (max3 < 0.1f * (float)max1) { ind3 = -1; }
  ind[0] = ind1; ind[1] = ind2; ind[2] = ind3;
}

// field `field` (an offsetof) of keypoint i of a keypoint array
template <class T>
__device__ __forceinline__ T kp_field(const uint8_t* kps, size_t i, size_t field) { return *(const T*)(kps + i * sizeof(orbx_keypoint) + field); }

// n16 16-byte pieces from src to the LDS block at dst: piece i lands at dst + 16 i (lane-linear inside a wave, as the LDS-DMA load writes)
template <int THREADS>
__device__ __forceinline__ void stage_dma(uint8_t* dst, const uint8_t* src, int n16) {
  for (int i0 = 0; i0 < n16; i0 += THREADS) {
    const int i = i0 + (int)threadIdx.x;
    uint8_t* d = dst + (size_t)(i0 + ((int)threadIdx.x & ~63)) * 16;   // wave-uniform; the hardware adds lane * 16
    if (i < n16)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + (size_t)i * 16),
                                       (__attribute__((address_space(3))) void*)d, 16, 0, 0);
  }
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// the nodes two FeatureVectors share, a thread per A node: emit(a0, a1, b0, b1), the two feature ranges (clamped), when neither is empty
template <int THREADS, class E>
__device__ __forceinline__ void common_nodes(const uint32_t* nodeA, const int32_t* pA, int kA, int totA, const uint32_t* nodeB, const int32_t* pB, int kB,
                                             int totB, E emit) {
  for (int ja = threadIdx.x; ja < kA; ja += THREADS) {
    const uint32_t node = nodeA[ja];
    int lo = 0, hi = kB;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (nodeB[mid] < node) lo = mid + 1; else hi = mid;
    }
    if (lo < kB && nodeB[lo] == node) {
      const int a0 = clampi(pA[ja], 0, totA), a1 = clampi(pA[ja + 1], 0, totA), b0 = clampi(pB[lo], 0, totB), b1 = clampi(pB[lo + 1], 0, totB);
      if (a1 > a0 && b1 > b0) emit(a0, a1, b0, b1);
    }
  }
}

// the wave's next item of a work list: lane 0 takes it from the LDS counter, wave-uniform
__device__ __forceinline__ int next_work(int* s_next) {
  int w = 0;
  if ((threadIdx.x & 63) == 0) w = atomicAdd(s_next, 1);
  return __builtin_amdgcn_readfirstlane(w);
}

// the exclusive prefix sum of v over the workgroup's WAVES waves, the sum in *total: a shuffle scan inside the wave, the wave sums through
// s_wave[WAVES], which may still be read from the previous use
template <int WAVES>
__device__ __forceinline__ int block_scan(int v, int* s_wave, int* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int p = __shfl_up(inc, o); if (lane >= o) inc += p; }
  __syncthreads();
  if (lane == 63) s_wave[wv] = inc;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < WAVES; w++) { const int s = s_wave[w]; before += w < wv ? s : 0; all += s; }
  *total = all;
  return before + inc - v;
}

}  // namespace dev
}  // namespace side
}  // namespace orbx
