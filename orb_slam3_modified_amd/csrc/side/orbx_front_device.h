// The projection-front core of liborbx_frustum.so, liborbx_project.so and liborbx_sim3.so: what their kernels and host twins share, stated
// once.  Their shape is B (pose, point list) items over one table of 48-byte map points, a lane per (item, slot), 256 slots a workgroup:
//   check_item           one workgroup per item: nslots and every index of the row's first nslots against npoints, before any of them
//                        addresses the table; the item's count becomes -1 (malformed) or 0
//   lane_of / finish     the lane's item and slot, the item's count read once (-1 stays -1), its index; the 32-byte row as two 16-byte
//                        stores, the count by a ballot, a popcount and one integer atomic per wave
//   count_level          the level as the number of ascending thresholds below the ratio, the level's scale factor picked on the way
// and the arithmetic every emitter is made of (sum3, cross3, transform) with the rows' words (Row, fw, iw).  The emitters themselves stay
// in their libraries: their gates differ on purpose.
// The part above __HIPCC__ is plain C++ (tests/support/front_check.cpp compiles it with the host compiler); the rest is device code.  It
// sits below csrc/, outside kernels_hash().
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../../include/orbx_project.h"

#ifdef __HIPCC__
#define ORBX_FRONT_HD __host__ __device__
#else
#define ORBX_FRONT_HD
#endif

namespace orbx {
namespace side {
namespace front {

constexpr int kThreads = 256;
constexpr int kMaxLevels = ORBX_FRUSTUM_MAX_LEVELS;
constexpr int kMaxT = kMaxLevels - 1;
static_assert(sizeof(orbx_frustum_point) == 48 && sizeof(orbx_project_item) == 128, "record sizes");

struct Row { uint32_t w[8]; };   // a row of any consumer, as its 32-bit words
ORBX_FRONT_HD inline uint32_t fw(float f) { return __builtin_bit_cast(uint32_t, f); }
ORBX_FRONT_HD inline uint32_t iw(int32_t i) { return (uint32_t)i; }

template <bool kTree>
ORBX_FRONT_HD inline float sum3(float a, float b, float c) { return kTree ? a + (b + c) : (a + b) + c; }

// Eigen's cross: (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0)
ORBX_FRONT_HD inline void cross3(const float* a, const float* b, float* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// Pc = T * P for a rigid pose (R, t, unit q)
template <bool kQuat, bool kTree>
ORBX_FRONT_HD inline void transform(const float* R, const float* t, const float* q, const float* P, float* Pc) {
  if (kQuat) {
    float uv[3], x[3];
    cross3(q, P, uv);
    for (int k = 0; k < 3; k++) uv[k] = uv[k] + uv[k];
    cross3(q, uv, x);
    for (int k = 0; k < 3; k++) Pc[k] = ((P[k] + q[3] * uv[k]) + x[k]) + t[k];
  } else {
    for (int k = 0; k < 3; k++) Pc[k] = sum3<kTree>(R[3 * k] * P[0], R[3 * k + 1] * P[1], R[3 * k + 2] * P[2]) + t[k];
  }
}

// The number of thresholds below ratio: T (kMaxT of them, +inf beyond nlevels - 2) ascends, so those are T[0 .. level); kScale: the level's
// scale factor (sf: kMaxLevels of them) is picked on the way.  Constant indices only: T and sf are kernel arguments.
template <bool kScale>
ORBX_FRONT_HD inline int count_level(const float* T, const float* sf, float ratio, float* scale) {
  int l = 0;
  float s = kScale ? sf[0] : 0.0f;
  if (ratio > 0.0f && ratio != INFINITY) {
#pragma unroll
    for (int n = 0; n < kMaxT; n++)
      if (ratio > T[n]) { l = n + 1; if (kScale) s = sf[n + 1]; }
  }
  *scale = s;
  return l;
}

#ifdef __HIPCC__
typedef uint32_t Words4 __attribute__((ext_vector_type(4)));

struct DeviceLevel {   // frustum's form returns the level alone
  const float* T; const float* sf;
  __device__ int operator()(float ratio) const { float s; return count_level<false>(T, sf, ratio, &s); }
  __device__ void operator()(float ratio, int* lvl, float* scale) const { *lvl = count_level<true>(T, sf, ratio, scale); }
};
struct DevicePoints {   // of the third 16 bytes only max_dist is fetched: the rest is padding
  const float4* t;
  __device__ orbx_frustum_point operator()(int idx) const {
    const float4 a = t[3 * (size_t)idx], b = t[3 * (size_t)idx + 1];
    const float max_dist = ((const float*)(t + 3 * (size_t)idx + 2))[0];
    return {{a.x, a.y, a.z}, a.w, {b.x, b.y, b.z}, b.w, max_dist, {0.0f, 0.0f, 0.0f}};
  }
};

// The check kernels' body for item blockIdx.x: `row` its slots of `stride` 32-bit words, the point's index the first; force_bad: the
// whole call is malformed (frustum's log_scale_factor)
__device__ inline void check_item(const int32_t* row, int stride, int nslots, int mcap, int npoints, bool force_bad, int32_t* nvalid) {
  int bad = force_bad || nslots < 0 || nslots > mcap;
  if (!bad)
    for (int j = threadIdx.x; j < nslots; j += kThreads) bad |= row[(size_t)j * stride] >= npoints;
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) *nvalid = bad ? -1 : 0;
}

// what the emitter kernels share: the lane's item and slot, its slot's words and index (or "none"), the row's stores and the count
struct Lane { int b, j, point; bool live, inside; size_t slot; const int32_t* s; };
__device__ inline Lane lane_of(const int32_t* slots, int stride, const int32_t* nslots, const int32_t* nvalid, int mcap, int chunks) {
  Lane l;
  l.b = (int)(blockIdx.x / (unsigned)chunks);
  l.j = (int)(blockIdx.x - (unsigned)l.b * (unsigned)chunks) * kThreads + (int)threadIdx.x;
  // -1 stays -1: a malformed item adds nothing; a sound one only grows from 0
  const bool bad = __hip_atomic_load(nvalid + l.b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0;
  const int n = bad ? 0 : nslots[l.b];
  l.inside = l.j < mcap;
  l.slot = (size_t)l.b * mcap + (l.inside ? l.j : 0);
  l.live = l.j < n;                       // n <= mcap
  l.s = slots + l.slot * stride;
  l.point = l.live ? l.s[0] : -1;
  return l;
}
__device__ inline void finish(const Lane& l, float4* out, int32_t* nvalid, const Row& r, bool valid, float* depths = nullptr, float depth = 0.0f) {
  if (l.inside) {
    Words4* const o = (Words4*)out + 2 * l.slot;   // native vectors: each half of the row stays one 16-byte store, whatever fields are constant
    o[0] = Words4{r.w[0], r.w[1], r.w[2], r.w[3]};
    o[1] = Words4{r.w[4], r.w[5], r.w[6], r.w[7]};
    if (depths) depths[l.slot] = depth;
  }
  const int count = __popcll(__ballot(valid));
  if (count > 0 && (threadIdx.x & 63) == 0) atomicAdd(nvalid + l.b, count);
}
#endif  // __HIPCC__

}  // namespace front
}  // namespace side
}  // namespace orbx
