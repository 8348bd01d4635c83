// The frame-grid window core of the four chained projection matchers (liborbx_localmatch.so, liborbx_lastmatch.so, liborbx_projmatch.so,
// liborbx_rigmatch.so): what k_local_match, k_last_match, k_proj_match and k_rig_match share, stated once.  Their shape is one 512-thread
// workgroup per item (the rig: two grids, a list per (point, camera), RES = 4 or 2 results a point):
//   check                the item's indices and counts, before any of them addresses memory (each kernel's own)
//   phase A, all waves   build_grid: the frame's keypoints as keys (cell << 16 | index), sorted (bitonic; the keys are unique, so the order is
//                        the frame grid's: cells x-major, then y, then ascending index), a 16-byte record per sorted position, the cells'
//                        starts by binary search.  A LANE PER POINT walks its window (walk) twice: once to count and, after scan_offsets,
//                        for a chunk of points whose lists fit the candidate room (chunk_end), once to write its list.
//   phase B, wave 0      the chain over the chunk's points in index order.  A step is open_top (64 lanes pass over the list's entries
//                        whose slot's bit is set and keep their smallest one or two (distance << 15 | position) keys, then a DPP
//                        min-reduction; open_second, behind the caller's gate, is the second), the kernel's accept test (ratio_test on two keys), bind by one lane (the slot into the point's
//                        results, the slot's bit) and publish.  The walk over a chunk's points (a lane preloads a point's list bounds and
//                        obs, readlane hands them out) and what a step writes beyond the bit are each kernel's own.
//   phase C, all waves   last_writer: kp_match[slot] = the LAST point that wrote it, kp_obs[slot] = that point's obs (not k_proj_match:
//                        there a slot is bound once, by the chain itself)
//   phase D, all waves   rotation_filter: the results' bins, ComputeThreeMaxima, the removal (not k_local_match)
// LDS path: the frame's descriptors, the grid, the offsets, the points' results and the candidate room in LDS (layout, rig_layout); global
// path: the descriptors where they lie, everything else in the workgroup's slice of the handle's scratch.
// The part above __HIPCC__ is plain C++ (tests/support/window_check.cpp compiles it with the host compiler); the rest is device code,
// included after orbx_pair_device.h.  It sits below csrc/, outside kernels_hash().
#pragma once
#include <climits>
#include <cstddef>
#include <cstdint>
#include <cstring>

#ifdef __HIPCC__
#define ORBX_WINDOW_HD __host__ __device__
#else
#define ORBX_WINDOW_HD
#endif

namespace orbx {
namespace side {
namespace win {

constexpr int kThreads = 512;             // 8 waves
constexpr int kLdsMax = 148 * 1024;       // dynamic LDS of one workgroup (160 KiB per CU, the static part is below 8 KiB)
constexpr int kMaxBlocks = 1024;          // workgroups of one launch on the LDS path
constexpr int kGlobalBlocks = 256;        // ... on the global path: each owns one slice of the scratch
constexpr int kGlobalRoom = 64 * 1024;    // candidates of one chunk on the global path (at least the capacity)
constexpr int kMaxCap = 32768;            // a key and a candidate hold a 15-bit index
constexpr int kMaxLevels = 16;
constexpr int kCols = 64, kRows = 48, kCells = kCols * kRows;
constexpr int kBins = 30;
constexpr int kNone = INT_MAX;            // no key
constexpr int kThHigh = 100;              // ORBmatcher::TH_HIGH
constexpr int kRecBytes = 16;             // sizeof(dev::Rec)
static_assert(kMaxCap == 1 << 15, "15-bit indices and positions");

// a / b for a normal a > 0 (64 and 48 here) and any b, rounded to nearest even as the float division is, by long division of the
// significands in integers: the division's own expansion would put fused multiply-adds into the code object.  A zero or subnormal b gives an
// infinity (64 / b is beyond FLT_MAX for every b below 1.9e-37), an infinite b a zero, a NaN itself.
ORBX_WINDOW_HD inline float div_rn(float a, float b) {
  uint32_t ua, ub;
  memcpy(&ua, &a, 4); memcpy(&ub, &b, 4);
  const uint32_t sign = ub & 0x80000000u, eb = (ub >> 23) & 0xFFu;
  uint32_t out;
  if (eb == 0xFFu) out = (ub & 0x7FFFFFu) ? ub : sign;
  else if (eb == 0u) out = sign | 0x7F800000u;
  else {
    uint32_t ma = (ua & 0x7FFFFFu) | 0x800000u;
    const uint32_t mb = (ub & 0x7FFFFFu) | 0x800000u;
    int e = (int)((ua >> 23) & 0xFFu) - (int)eb;
    if (ma < mb) { ma <<= 1; e--; }        // 1 <= ma / mb < 2
    uint32_t rem = ma - mb, q = 1u;        // the quotient's leading bit, then 23 more and a guard bit
#pragma unroll
    for (int i = 0; i < 24; i++) {
      rem <<= 1; q <<= 1;
      if (rem >= mb) { rem -= mb; q |= 1u; }
    }
    uint32_t m = q >> 1;
    if ((q & 1u) && (rem != 0u || (m & 1u))) m++;
    if (m == 0x1000000u) { m >>= 1; e++; }
    const int be = e + 127;                // at least 5 for a >= 48 and a normal b
    out = be >= 255 ? sign | 0x7F800000u : be < 1 ? sign : sign | (uint32_t)be << 23 | (m & 0x7FFFFFu);
  }
  float r;
  memcpy(&r, &out, 4);
  return r;
}

// One item's arrays, as offsets in the LDS block resp. the scratch slice (16-byte aligned).  A grid's block: the sorted
// (cell << 16 | index) keys of a frame's keypoints, their records in the same order, the first sorted position of every cell.
struct Bump {
  size_t o = 0;
  ORBX_WINDOW_HD size_t add(size_t bytes) { const size_t at = o; o = (o + bytes + 15) & ~(size_t)15; return at; }
};
struct GridLay { size_t keys, recs, cstart; };
ORBX_WINDOW_HD inline GridLay grid_layout(Bump& b, int cap, int p2) {
  GridLay g;
  g.keys = b.add((size_t)p2 * 4);
  g.recs = b.add((size_t)cap * kRecBytes);
  g.cstart = b.add((size_t)(kCells + 1) * 2);
  return g;
}
struct Lay { size_t desc; GridLay grid; size_t offs, res, cand, fixed; };
ORBX_WINDOW_HD inline Lay layout(int cap, int mcap, int p2, bool lds) {
  Lay l;
  Bump b;
  l.desc = b.add(lds ? (size_t)cap * 32 : 0);
  l.grid = grid_layout(b, cap, p2);
  l.offs = b.add((size_t)(mcap + 1) * 4);   // first candidate of every point (exclusive scan of the counts)
  l.res = b.add((size_t)mcap * 4);          // the keypoint a point was accepted with (rotation_filter: its bin + 1 above bit 16), -1 without
  l.cand = l.fixed = b.o;
  return l;
}
// the rig's: two grids
struct RigLay { size_t desc_l, desc_r; GridLay grid_l, grid_r; size_t offs, res, cand, fixed; };
ORBX_WINDOW_HD inline RigLay rig_layout(int cap_l, int cap_r, int mcap, int p2l, int p2r, bool lds) {
  RigLay l;
  Bump b;
  l.desc_l = b.add(lds ? (size_t)cap_l * 32 : 0);
  l.desc_r = b.add(lds ? (size_t)cap_r * 32 : 0);
  l.grid_l = grid_layout(b, cap_l, p2l);
  l.grid_r = grid_layout(b, cap_r, p2r);
  l.offs = b.add((size_t)(2 * mcap + 1) * 4);   // first candidate of every (point, camera) list
  l.res = b.add((size_t)mcap * 16);             // the slots a point wrote: four (entry 1) or two (entry 2) a point, -1 without
  l.cand = l.fixed = b.o;
  return l;
}

#ifdef __HIPCC__
using namespace orbx::side::dev;
static_assert(sizeof(Rec) == kRecBytes, "layout's record");

constexpr size_t kX = offsetof(orbx_keypoint, x), kY = offsetof(orbx_keypoint, y), kOctave = offsetof(orbx_keypoint, octave),
                 kAngle = offsetof(orbx_keypoint, angle);

struct Arrays { uint32_t* keys; Rec* recs; uint16_t* cstart; int32_t* offs; int32_t* res; uint32_t* cand; };
template <class L>                        // Lay or RigLay: a grid of the layout with the layout's offsets, results and candidate room
__device__ __forceinline__ Arrays arrays(uint8_t* base, const L& lay, const GridLay& g) {
  return {(uint32_t*)(base + g.keys), (Rec*)(base + g.recs), (uint16_t*)(base + g.cstart), (int32_t*)(base + lay.offs), (int32_t*)(base + lay.res),
          (uint32_t*)(base + lay.cand)};
}

// the level table into LDS: constant indices into the kernel's arguments
__device__ __forceinline__ void load_levels(float* s_sf, const float (&sf)[kMaxLevels]) {
  const int tid = threadIdx.x;
  if (tid < kMaxLevels) {
    float v = 0.0f;
#pragma unroll
    for (int l = 0; l < kMaxLevels; l++)
      if (tid == l) v = sf[l];
    s_sf[tid] = v;
  }
}

__device__ __forceinline__ void set_bit(int32_t* bits, int i) { atomicOr(&bits[i >> 5], (int)(1u << (i & 31))); }

// a frame's grid from its bounds {min_x, min_y, max_x, max_y} (src/Frame.cc:153-160)
struct Grid { float minX, minY, invW, invH; };
__device__ __forceinline__ Grid frame_grid(const float* b) {
  return {b[0], b[1], div_rn((float)kCols, b[2] - b[0]), div_rn((float)kRows, b[3] - b[1])};
}

// Phase A's grid of the frame's n keypoints: keys, records (ur null: -1) and cell starts.  It begins with a barrier, so what the caller
// initialised for each(i), the kernel's own work in the same trip over the keypoints (its hidden / taken bit), is seen; it ends with one.
template <int THREADS, class E>
__device__ __forceinline__ void build_grid(const Grid& G, const uint8_t* kp, const float* ur, int n, const Arrays& A, E each) {
  __shared__ int s_cnt;
  const int tid = threadIdx.x;
  uint32_t* const keys = A.keys;
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  for (int i = tid; i < n; i += THREADS) {
    each(i);
    // Frame::PosInGrid (src/Frame.cc:725-735)
    const float fx = roundf((kp_field<float>(kp, i, kX) - G.minX) * G.invW), fy = roundf((kp_field<float>(kp, i, kY) - G.minY) * G.invH);
    if (!(fx >= 0.0f && fx < (float)kCols && fy >= 0.0f && fy < (float)kRows)) continue;   // outside the grid (or NaN): in no cell
    const int k = atomicAdd(&s_cnt, 1);    // k < n <= cap <= p2
    keys[k] = (uint32_t)((int)fx * kRows + (int)fy) << 16 | (uint32_t)i;
  }
  __syncthreads();
  const int n0 = s_cnt;                    // the frame's keypoints inside the grid
  int n2 = 2;
  while (n2 < n0) n2 <<= 1;                // n2 <= p2
  for (int i = n0 + tid; i < n2; i += THREADS) keys[i] = 0xFFFFFFFFu;
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (n2 >> 1); t += THREADS) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const uint32_t a = keys[i], c = keys[l];
        if ((a > c) == ((i & k) == 0)) { keys[i] = c; keys[l] = a; }
      }
      __syncthreads();
    }
  for (int j = tid; j < n0; j += THREADS) {
    const size_t i = keys[j] & 0xFFFFu;
    A.recs[j] = Rec{kp_field<float>(kp, i, kX), kp_field<float>(kp, i, kY), kp_field<int32_t>(kp, i, kOctave), ur ? ur[i] : -1.0f};
  }
  for (int c = tid; c <= kCells; c += THREADS) {
    const uint32_t want = (uint32_t)c << 16;
    int lo = 0, hi = n0;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (keys[mid] < want) lo = mid + 1; else hi = mid;
    }
    A.cstart[c] = (uint16_t)lo;            // <= 32768
  }
  __syncthreads();
}

// Frame::GetFeaturesInArea(x, y, r, minLevel, maxLevel) (src/Frame.cc:657-723) over the sorted records: emit(record, index) for every
// candidate, in the reference's order.  BOTH: the caller's maxLevel is never negative, so bCheckLevels holds and both bounds are tested
// (the local and the projection matcher: the literal form's tests in the inner loop cost them 10 and 16 % of phase A).
template <bool BOTH, class F>
__device__ __forceinline__ void walk(const Grid& G, float x, float y, float r, int minLevel, int maxLevel, const Arrays& A, F emit) {
  const int x0 = max(0, (int)floorf((x - G.minX - r) * G.invW));
  if (x0 >= kCols) return;
  const int x1 = min(kCols - 1, (int)ceilf((x - G.minX + r) * G.invW));
  if (x1 < 0) return;
  const int y0 = max(0, (int)floorf((y - G.minY - r) * G.invH));
  if (y0 >= kRows) return;
  const int y1 = min(kRows - 1, (int)ceilf((y - G.minY + r) * G.invH));
  if (y1 < 0) return;
  if (y1 < y0) return;                     // an empty range of rows (the reference's inner loop does not run)
  const bool levels = BOTH || minLevel > 0 || maxLevel >= 0;   // bCheckLevels
  for (int ix = x0; ix <= x1; ix++) {      // the cells (ix, y0 .. y1) are neighbours in the sorted keys
    const int j1 = A.cstart[ix * kRows + y1 + 1];
    for (int j = A.cstart[ix * kRows + y0]; j < j1; j++) {
      const Rec c = A.recs[j];
      if (levels) {
        if (c.octave < minLevel) continue;
        if ((BOTH || maxLevel >= 0) && c.octave > maxLevel) continue;
      }
      if (fabsf(c.x - x) < r && fabsf(c.y - y) < r) emit(c, (int)(A.keys[j] & 0xFFFFu));
    }
  }
}

// offs[0 .. m) from counts to their exclusive prefix sums, in place; a barrier first (the counts are complete), the caller's after it
template <int THREADS>
__device__ __forceinline__ void scan_offsets(int32_t* offs, int m) {
  __shared__ int s_scan[THREADS];
  const int tid = threadIdx.x, per = (m + THREADS - 1) / THREADS;
  const int lo = min(m, tid * per), hi = min(m, lo + per);
  __syncthreads();
  int s = 0;
  for (int i = lo; i < hi; i++) s += offs[i];
  s_scan[tid] = s;
  __syncthreads();
  for (int d = 1; d < THREADS; d <<= 1) {
    const int v = tid >= d ? s_scan[tid - d] : 0;
    __syncthreads();
    s_scan[tid] += v;
    __syncthreads();
  }
  int run = s_scan[tid] - s;
  for (int i = lo; i < hi; i++) { const int c = offs[i]; offs[i] = run; run += c; }
}

// the chunk of points from q0, LISTS lists a point: the largest q1 <= nq with offs[LISTS q1] - offs[LISTS q0] <= room.  A chunk ends
// between points; one point's lists (<= the slots <= room) always fit
template <int LISTS = 1>
__device__ __forceinline__ int chunk_end(const int32_t* offs, int q0, int nq, int room) {
  const int e0 = offs[LISTS * q0];
  int lo = q0 + 1, hi = nq;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (offs[LISTS * mid] - e0 <= room) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// ---- phase B, wave 0.  The chain's state (the bits, the points' results) is written by one lane and read by the wave's other lanes in
// the next step: ld / st, and publish between a step's binds and the next step's loads.
// The wave's smallest (distance << 15 | position) key among the list's entries cand[b0 .. b0 + cnt) whose slot (base + index) is open: its
// bit in `bits` is clear; kNone without one (kNone >> 15 is above every distance).  All 64 lanes call it.  `mine`, for a two-key caller:
// the lane's own two smallest keys, from which open_second forms the wave's second smallest once the caller's gate on the first has
// passed: the caller's branch stands between the two reductions.
struct LaneKeys { int k1, k2; };
__device__ __forceinline__ int open_top(const uint32_t* cand, int b0, int cnt, int base, const int32_t* bits, int lane, LaneKeys* mine = nullptr) {
  int k1 = kNone, k2 = kNone;
  for (int j = lane; j < cnt; j += 64) {
    const uint32_t e = cand[b0 + j];
    const int s = base + (int)(e & 0x7FFFu);
    if ((ld(bits + (s >> 5)) >> (s & 31)) & 1) continue;
    const int key = (int)((e >> 15) & 0x1FFu) << 15 | j;
    const int hi = max(k1, key);
    k1 = min(k1, key);
    k2 = min(k2, hi);
  }
  if (mine) *mine = {k1, k2};
  return wave_min(k1);
}
// positions are unique, so one lane holds m1: its second key stands in, every other lane's first
__device__ __forceinline__ int open_second(const LaneKeys& mine, int m1) { return wave_min(mine.k1 == m1 ? mine.k2 : mine.k1); }

// src/ORBmatcher.cc:117-130 resp. :193-196 on the two keys, whose entries carry the octaves above bit 24: 0 nothing (no open candidate, or
// bestDist > kThHigh), 1 the `continue` (equal octaves and bestDist > mfNNratio * bestDist2), 2 the octaves differ or bestDist <=
// mfNNratio * bestDist2, 3 neither comparison holds (a NaN ratio).  *idx: the best entry's index, for every outcome but 0.
__device__ __forceinline__ int ratio_test(const uint32_t* cand, int b0, int m1, int m2, float ratio, int* idx) {
  if ((m1 >> 15) > kThHigh) return 0;      // kNone too
  const uint32_t e1 = cand[b0 + (m1 & 0x7FFF)];
  const int best = m1 >> 15, level1 = (int)(e1 >> 24 & 31u);
  int second = 256, level2 = 31;           // bestDist2 = 256, bestLevel2 = -1
  if (m2 != kNone) {
    second = m2 >> 15;
    level2 = (int)(cand[b0 + (m2 & 0x7FFF)] >> 24 & 31u);
  }
  *idx = (int)(e1 & 0x7FFFu);
  if (level1 != level2) return 2;          // first: most steps end here, before the float compare
  const float lim = ratio * (float)second;
  return (float)best > lim ? 1 : (float)best <= lim ? 2 : 3;
}

// One lane: the point's result *res = slot, and the slot's bit set (its new holder has obs > 0 observations) or cleared.  CLEAR = false:
// the slot was open, as in the one-camera matchers, so clearing is a no-op and the bit's word is touched for obs > 0 alone (the
// unconditional load and store cost k_local_match and k_last_match 3 to 4 % of a call: profiles/chain_core_refactor.txt).
template <bool CLEAR>
__device__ __forceinline__ void bind(int32_t* bits, int32_t* res, int slot, int obs) {
  st(res, slot);
  if (!CLEAR && obs <= 0) return;
  const int w = ld(bits + (slot >> 5)), bit = (int)(1u << (slot & 31));
  st(bits + (slot >> 5), obs > 0 ? w | bit : w & ~bit);
}
// all lanes, after a step's binds: the stores are done before the next step's loads
__device__ __forceinline__ void publish() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }

// Phase C, all waves: match[slot] = the LAST of the nq points that wrote the slot (res: RES results a point, a slot below `slots` or -1;
// an integer maximum over the writers' indices, so the order does not matter), then obs[slot] = obs_of(that point).  A barrier lies
// between the two; the caller's follows.
template <int THREADS, int RES, class O>
__device__ __forceinline__ void last_writer(const int32_t* res, int nq, int slots, int32_t* match, int32_t* obs, O obs_of) {
  const int tid = threadIdx.x;
  for (int e = tid; e < RES * nq; e += THREADS) {
    const int s = res[e];
    if (s >= 0 && s < slots) __hip_atomic_fetch_max(match + s, e / RES, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  for (int s = tid; s < slots; s += THREADS) {
    const int q = __hip_atomic_load(match + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (q >= 0 && q < nq) obs[s] = obs_of(q);
  }
}

// Phase D, all waves: the rotation histogram of the nq points' results (res: RES results a point, a slot below `slots` or -1; angle(q) the
// point's angle, angle_of(slot) the slot's keypoint's) by integer adds into 30 LDS counters, ComputeThreeMaxima
// (src/ORBmatcher.cc:2012-2053) by one lane, then remove(slot) for every entry of another bin.  Returns the number of entries removed.
// Begins with a barrier and ends with one.
template <int THREADS, int RES, class A, class K, class R>
__device__ __forceinline__ int rotation_filter(int32_t* res, int nq, int slots, A angle, K angle_of, R remove) {
  __shared__ int s_hist[32], s_ind[3], s_removed;
  const int tid = threadIdx.x;
  if (tid < 32) s_hist[tid] = 0;
  if (tid == 0) s_removed = 0;
  __syncthreads();
  for (int e = tid; e < RES * nq; e += THREADS) {
    const int i = res[e];
    if (i < 0 || i >= slots) continue;
    const int bin = rot_bin(angle(e / RES), angle_of(i));
    if (bin >= 0) atomicAdd(&s_hist[bin], 1);
    res[e] = i | (bin + 1) << 16;          // i < 32768; bin + 1 in 0 .. 30
  }
  __syncthreads();
  if (tid == 0) {
    int ind1 = -1, ind2 = -1, ind3 = -1, max1 = 0, max2 = 0, max3 = 0;
    for (int i = 0; i < kBins; i++) {
      const int s = s_hist[i];
      if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
      else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
      else if (s > max3) { max3 = s; ind3 = i; }
    }
    if ((float)max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
    else if ((float)max3 < 0.1f * (float)max1) { ind3 = -1; }
    s_ind[0] = ind1; s_ind[1] = ind2; s_ind[2] = ind3;
  }
  __syncthreads();
  const int ind1 = s_ind[0], ind2 = s_ind[1], ind3 = s_ind[2];
  for (int e = tid; e < RES * nq; e += THREADS) {
    const int r = res[e];
    if (r < 0) continue;
    const int bin = (r >> 16) - 1, i = r & 0xFFFF;   // i < slots: only such results were given a bin
    if (bin < 0 || bin == ind1 || bin == ind2 || bin == ind3) continue;
    remove(i);
    atomicAdd(&s_removed, 1);
  }
  __syncthreads();
  return s_removed;
}
#endif  // __HIPCC__

}  // namespace win
}  // namespace side
}  // namespace orbx
