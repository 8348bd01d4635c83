// The batched relocalization and Sim3 matchers (include/orbx_projmatch.h): ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF,
// sAlreadyFound, th, ORBdist) (src/ORBmatcher.cc:1889-2010, kind 0) and SearchByProjection(KeyFrame*, Sim3f& Scw, vpPoints[, vpPointsKFs],
// vpMatched[, vpMatchedKF], th, ratioHamming) (:427-532, :534-646, kind 1) for B (frame, projected points) items on the keypoints and
// descriptors a batch extraction left in HBM and the points' descriptors in the pool ComputeDistinctiveDescriptors fills.
//
// k_proj_match<LDS>: one workgroup of 8 waves per item (a grid of at most kMaxBlocks workgroups walks the items); the shape is
// csrc/lastmatch/orbx_lastmatch.hip's with less in it, written out again here (its pieces do not move without changing that kernel's
// assembly).
//   check, all waves     the item's frame, count, npts, kind and th and every valid point's level and pool row, before any of them
//                        addresses memory.
//   phase A, all waves   the frame's keypoints as keys (cell << 16 | index), sorted (bitonic, keys are unique: the order is the frame grid's:
//                        cells x-major, then y, then ascending index), a 16-byte record {x, y, octave, -} per sorted position, the cells'
//                        starts by binary search.  A LANE PER POINT walks its window twice: once to count, and after a workgroup scan, for a
//                        chunk of points whose lists fit the candidate room, once to write its list with the point's descriptor in 8
//                        registers.  A candidate is one word: index (15 bits), Hamming distance (9).  The level range [level - 1,
//                        level + 1 - kind] and the strict window test are applied here (for kind 1 the reference applies the range in its
//                        walk over an unfiltered list, :509 / :622: the same keypoints in the same order); the taken test is the chain's.
//                        (Only a best is kept, so entries above the item's max_dist could be left out of the lists; they are not: see
//                        DESIGN.md section 21.)
//   phase B, wave 0      the chain over the chunk's points in index order: lane j holds candidate j (+ 64 per trip), drops the entries whose
//                        keypoint is taken (a bit per keypoint in LDS, from the kp_taken row, set on every acceptance), keeps its smallest
//                        (distance << 15 | position) key; one DPP min-reduction gives the wave's smallest: the first in walk order among
//                        equal distances.  The accept test, a float compare against the item's max_dist, is wave-uniform; one lane writes
//                        kp_match, records the point's keypoint and sets the bit.  No descriptor and no keypoint is read here.  A and B
//                        repeat per chunk: the distances do not depend on the chain, so where the chunks are cut changes nothing.
//   phase D, all waves   kind 0 under check_orientation: every accepted point's bin (integer adds into 30 LDS counters),
//                        ComputeThreeMaxima by one lane, then every entry of another bin writes kp_match = -2 and counts itself (an integer
//                        add).  A keypoint is bound at most once per row, so every entry is a keypoint of its own.
// LDS path: the frame's descriptors (16-byte LDS-DMA loads), the grid, the offsets, the points' results and the candidate room in LDS.
// Global path (sizes that need more LDS than the handle's limit): the descriptors where they lie, everything else in the workgroup's slice of
// the handle's scratch.  The taken bits are 4 KiB of static LDS on both paths.
// The float expressions are compiled with -ffp-contract=off: every operation is rounded by itself, as the specification states them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>

#include "../side/orbx_handle.h"
#include "../side/orbx_pair_device.h"
#include "../../../include/orbx_projmatch.h"

namespace {

using namespace orbx::side::dev;          // ld / st on the chain's state: written by one lane, read by the wave's other lanes in the next step

constexpr int kThreads = 512;             // 8 waves
constexpr int kLdsMax = 148 * 1024;       // dynamic LDS of one workgroup (160 KiB per CU, the static part is below 8 KiB)
constexpr int kMaxBlocks = 1024;          // workgroups of one launch on the LDS path
constexpr int kGlobalBlocks = 256;        // ... on the global path: each owns one slice of the scratch
constexpr int kGlobalRoom = 64 * 1024;    // candidates of one chunk on the global path (at least the capacity)
constexpr int kMaxCap = ORBX_PROJMATCH_MAX_CAPACITY;   // a key and a candidate hold a 15-bit index
constexpr int kCols = 64, kRows = 48, kCells = kCols * kRows;
constexpr int kBins = 30;
constexpr int kNone = INT_MAX;            // no key
static_assert(kMaxCap == 32768, "15-bit indices and positions");
static_assert(sizeof(orbx_projmatch_item) == 16 && sizeof(orbx_projmatch_point) == 32, "the ABI's records");

constexpr size_t kX = offsetof(orbx_keypoint, x), kY = offsetof(orbx_keypoint, y), kOctave = offsetof(orbx_keypoint, octave),
                 kAngle = offsetof(orbx_keypoint, angle);

// a / b for a normal a > 0 (64 and 48 here) and any b, rounded to nearest even as the float division is, by long division of the
// significands in integers: the division's own expansion would put fused multiply-adds into the code object.  A zero or subnormal b gives an
// infinity (64 / b is beyond FLT_MAX for every b below 1.9e-37), an infinite b a zero, a NaN itself.
__host__ __device__ inline float div_rn(float a, float b) {
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

struct Args {
  const uint8_t* kps; const uint8_t* desc; const int32_t* counts; const float* bounds;
  const orbx_projmatch_item* items; const orbx_projmatch_point* pts; const int32_t* npts; const uint8_t* pdesc;
  const uint8_t* kp_taken; int32_t* kp_match; int32_t* nmatches;
  uint8_t* scratch; size_t scratch_stride;
  int nframes, cap, nitems, mcap, npoints, nlevels, p2, room, check_ori;
  float sf[ORBX_PROJMATCH_MAX_LEVELS];
};

// one item's arrays, as offsets in the LDS block resp. the scratch slice (16-byte aligned)
struct Lay { size_t desc, keys, recs, cstart, offs, res, cand, fixed; };
__host__ __device__ inline Lay layout(int cap, int mcap, int p2, bool lds) {
  Lay l;
  size_t o = 0;
  auto add = [&](size_t bytes) { const size_t at = o; o = (o + bytes + 15) & ~(size_t)15; return at; };
  l.desc = add(lds ? (size_t)cap * 32 : 0);
  l.keys = add((size_t)p2 * 4);             // sorted (cell << 16 | index) of the frame's keypoints
  l.recs = add((size_t)cap * sizeof(Rec));  // their records, in the same order
  l.cstart = add((size_t)(kCells + 1) * 2); // first sorted position of every cell
  l.offs = add((size_t)(mcap + 1) * 4);     // first candidate of every point (exclusive scan of the counts)
  l.res = add((size_t)mcap * 4);            // the keypoint a point was accepted with (and, from phase D, its bin + 1 above bit 16), -1 without
  l.cand = o;
  l.fixed = o;
  return l;
}

// Frame::GetFeaturesInArea(x, y, r, lo, hi) with hi >= 0 (src/Frame.cc:657-723) over the sorted records: emit(index) for every candidate,
// in the reference's order.  bCheckLevels is true for every call made here; for kind 1 (lo, hi) = (level - 1, level) is the test of the
// reference's own walk over KeyFrame::GetFeaturesInArea's unfiltered list (src/ORBmatcher.cc:509, :622).
template <class F>
__device__ __forceinline__ void walk(float minX, float minY, float invW, float invH, float x, float y, float r, int lo, int hi,
                                     const uint16_t* cstart, const Rec* recs, const uint32_t* keys, F emit) {
  const int x0 = max(0, (int)floorf((x - minX - r) * invW));
  if (x0 >= kCols) return;
  const int x1 = min(kCols - 1, (int)ceilf((x - minX + r) * invW));
  if (x1 < 0) return;
  const int y0 = max(0, (int)floorf((y - minY - r) * invH));
  if (y0 >= kRows) return;
  const int y1 = min(kRows - 1, (int)ceilf((y - minY + r) * invH));
  if (y1 < 0) return;
  if (y1 < y0) return;                     // an empty range of rows (the reference's inner loop does not run)
  for (int ix = x0; ix <= x1; ix++) {      // the cells (ix, y0 .. y1) are neighbours in the sorted keys
    const int j1 = cstart[ix * kRows + y1 + 1];
    for (int j = cstart[ix * kRows + y0]; j < j1; j++) {
      const Rec c = recs[j];
      if (c.octave < lo || c.octave > hi) continue;
      if (fabsf(c.x - x) < r && fabsf(c.y - y) < r) emit((int)(keys[j] & 0xFFFFu));
    }
  }
}

// a point's window: th times the level's scale (:489, :602, :1937); the level range is [level - 1, level + up]
struct Pt { float x, y, radius; int level, point; bool live; };
__device__ __forceinline__ Pt load_point(const orbx_projmatch_point* p, const float* s_sf, float th) {
  const uint4* const rp = (const uint4*)p;
  const uint4 lo = rp[0];
  const uint2 hi = *(const uint2*)(rp + 1);
  Pt t;
  t.x = __uint_as_float(lo.x); t.y = __uint_as_float(lo.y);
  t.level = (int)lo.w;
  t.point = (int)hi.x;
  // valid, and finite: a NaN fails every comparison (the reference leaves a non-finite projection undefined; here it has no candidate)
  t.live = hi.y != 0u && fabsf(t.x) < INFINITY && fabsf(t.y) < INFINITY;
  t.radius = 0.0f;
  if (t.live) t.radius = th * s_sf[t.level];       // the level is one of the table's: the check
  return t;
}

template <bool LDS>
__global__ __launch_bounds__(kThreads) void k_proj_match(Args g) {
  extern __shared__ __align__(16) uint8_t smem[];
  __shared__ int s_cnt, s_bad, s_removed;
  __shared__ int s_hist[32], s_ind[3];
  __shared__ int s_scan[kThreads];
  __shared__ int32_t s_taken[kMaxCap / 32];    // bit i: keypoint i holds a map point
  __shared__ float s_sf[ORBX_PROJMATCH_MAX_LEVELS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int cap = g.cap, mcap = g.mcap;
  const Lay L = layout(cap, mcap, g.p2, LDS);
  uint8_t* const base = LDS ? smem : g.scratch + (size_t)blockIdx.x * g.scratch_stride;
  uint32_t* const keys = (uint32_t*)(base + L.keys);
  Rec* const recs = (Rec*)(base + L.recs);
  uint16_t* const cstart = (uint16_t*)(base + L.cstart);
  int32_t* const offs = (int32_t*)(base + L.offs);
  int32_t* const res = (int32_t*)(base + L.res);
  uint32_t* const cand = (uint32_t*)(base + L.cand);

  if (tid < ORBX_PROJMATCH_MAX_LEVELS) {   // the level table: constant indices into the kernel's arguments
    float v = 0.0f;
#pragma unroll
    for (int l = 0; l < ORBX_PROJMATCH_MAX_LEVELS; l++)
      if (tid == l) v = g.sf[l];
    s_sf[tid] = v;
  }

  for (int b = blockIdx.x; b < g.nitems; b += gridDim.x) {
    __syncthreads();                       // the previous item's shared state has been read
    int32_t* const omatch = g.kp_match + (size_t)b * cap;
    const orbx_projmatch_point* const pts = g.pts + (size_t)b * mcap;
    // ---- the check: nothing below addresses memory with a value that was not tested here
    const int f = g.items[b].frame, kind = g.items[b].kind, npts = g.npts[b];
    const float th = g.items[b].th, max_dist = g.items[b].max_dist;
    bool ok = f >= 0 && f < g.nframes && npts >= 0 && npts <= mcap && kind >= 0 && kind <= 1 && fabsf(th) < INFINITY;
    int n = 0;
    if (ok) {
      n = g.counts[2 * f];
      ok = n >= 0 && n <= cap;
    }
    if (tid == 0) { s_cnt = 0; s_bad = 0; s_removed = 0; }
    if (tid < 32) s_hist[tid] = 0;
    for (int i = tid; i < cap; i += kThreads) omatch[i] = -1;
    __syncthreads();
    if (ok) {                              // uniform over the workgroup
      bool bad = false;
      for (int q = tid; q < npts; q += kThreads) {
        const int level = (int)((const uint4*)(pts + q))[0].w;
        const uint2 hi = *(const uint2*)((const uint4*)(pts + q) + 1);
        bad |= hi.y != 0u && (level < 0 || level >= g.nlevels || (int)hi.x < 0 || (int)hi.x >= g.npoints);
      }
      if (bad) s_bad = 1;
    }
    __syncthreads();
    if (!ok || s_bad) {                    // uniform over the workgroup: a row of -1
      if (tid == 0) g.nmatches[b] = -1;
      continue;
    }
    const int up = 1 - kind;               // kind 0: [level - 1, level + 1] (:1939); kind 1: [level - 1, level] (:509, :622)
    const size_t of = (size_t)f * cap;
    const uint8_t* const kp = g.kps + of * sizeof(orbx_keypoint);
    const uint8_t* const taken = g.kp_taken ? g.kp_taken + (size_t)b * cap : nullptr;
    const uint8_t* const desc = LDS ? base + L.desc : g.desc + of * 32;
    const float minX = g.bounds[4 * f], minY = g.bounds[4 * f + 1];
    const float invW = div_rn((float)kCols, g.bounds[4 * f + 2] - minX), invH = div_rn((float)kRows, g.bounds[4 * f + 3] - minY);   // src/Frame.cc:153-160

    // ---- phase A: the frame's grid
    if (LDS) stage_dma<kThreads>(base + L.desc, g.desc + of * 32, n * 2);
    for (int w = tid; w < kMaxCap / 32; w += kThreads) s_taken[w] = 0;
    for (int q = tid; q < npts; q += kThreads) res[q] = -1;
    __syncthreads();
    for (int i = tid; i < n; i += kThreads) {
      if (taken && taken[i]) atomicOr(&s_taken[i >> 5], (int)(1u << (i & 31)));
      // Frame::PosInGrid (src/Frame.cc:725-735)
      const float fx = roundf((kp_field<float>(kp, i, kX) - minX) * invW), fy = roundf((kp_field<float>(kp, i, kY) - minY) * invH);
      if (!(fx >= 0.0f && fx < (float)kCols && fy >= 0.0f && fy < (float)kRows)) continue;   // outside the grid (or NaN): in no cell
      const int k = atomicAdd(&s_cnt, 1);  // k < n <= cap <= p2
      keys[k] = (uint32_t)((int)fx * kRows + (int)fy) << 16 | (uint32_t)i;
    }
    __syncthreads();
    const int n0 = s_cnt;                  // the frame's keypoints inside the grid
    int n2 = 2;
    while (n2 < n0) n2 <<= 1;              // n2 <= p2
    for (int i = n0 + tid; i < n2; i += kThreads) keys[i] = 0xFFFFFFFFu;
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = tid; t < (n2 >> 1); t += kThreads) {
          const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
          const uint32_t a = keys[i], c = keys[l];
          if ((a > c) == ((i & k) == 0)) { keys[i] = c; keys[l] = a; }
        }
        __syncthreads();
      }
    for (int j = tid; j < n0; j += kThreads) {
      const size_t i = keys[j] & 0xFFFFu;
      recs[j] = Rec{kp_field<float>(kp, i, kX), kp_field<float>(kp, i, kY), kp_field<int32_t>(kp, i, kOctave), -1.0f};
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

    // ---- phase A: every point's candidate count, then the offsets
    for (int q = tid; q <= npts; q += kThreads) {
      int c = 0;
      if (q < npts) {
        const Pt t = load_point(pts + q, s_sf, th);
        if (t.live) walk(minX, minY, invW, invH, t.x, t.y, t.radius, t.level - 1, t.level + up, cstart, recs, keys, [&](int) { c++; });
      }
      offs[q] = c;
    }
    __syncthreads();
    {
      const int m = npts + 1, per = (m + kThreads - 1) / kThreads;
      const int lo = min(m, tid * per), hi = min(m, lo + per);
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

    // ---- chunks of points whose candidates fit the room: lists with distances (all waves), then the chain (wave 0)
    int nm = 0;                            // wave 0's count of acceptances
    for (int q0 = 0; q0 < npts;) {
      const int e0 = offs[q0];
      int q1;
      {                                    // the largest q1 with offs[q1] - e0 <= room; one point's list (<= cap <= room) always fits
        int lo = q0 + 1, hi = npts;
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
          const Pt t = load_point(pts + q, s_sf, th);
          const D8 qd = load_desc(g.pdesc + (size_t)t.point * 32);   // the pool row is below npoints: the check
          walk(minX, minY, invW, invH, t.x, t.y, t.radius, t.level - 1, t.level + up, cstart, recs, keys, [&](int i) {
            if (k < kend && k < tot) {
              const int d = hamming(qd, load_desc(desc + (size_t)i * 32));
              cand[k] = (uint32_t)i | (uint32_t)d << 15;
            }
            k++;
          });
        }
      }
      __syncthreads();

#ifndef ORBX_PROJMATCH_NO_CHAIN            // (a timing build without phase B: tools/projmatch_times.py; its results are not the specification's)
      if (tid < 64) {                      // ---- phase B
        for (int c0 = q0; c0 < q1; c0 += 64) {
          const int cn = min(64, q1 - c0);
          int l_b = 0, l_n = 0;
          if (lane < cn) { l_b = offs[c0 + lane] - e0; l_n = offs[c0 + lane + 1] - e0 - l_b; }
          for (int i = 0; i < cn; i++) {
            const int cnt = __builtin_amdgcn_readlane(l_n, i);
            if (cnt <= 0) continue;
            const int b0 = __builtin_amdgcn_readlane(l_b, i);
            int k1 = kNone;                // the lane's smallest (distance << 15 | position)
            for (int j = lane; j < cnt; j += 64) {
              const uint32_t e = cand[b0 + j];
              const int idx = (int)(e & 0x7FFFu);
              if ((ld(s_taken + (idx >> 5)) >> (idx & 31)) & 1) continue;   // :504, :1952
              k1 = min(k1, (int)((e >> 15) & 0x1FFu) << 15 | j);
            }
            const int m1 = wave_min(k1);
            if (m1 == kNone || !((float)(m1 >> 15) <= max_dist)) continue;   // :523, :636, :1966; a NaN limit accepts nothing
            if (lane == 0) {
              const int idx = (int)(cand[b0 + (m1 & 0x7FFF)] & 0x7FFFu);     // below n: a candidate is a keypoint of the grid
              omatch[idx] = c0 + i;
              st(res + c0 + i, idx);
              st(s_taken + (idx >> 5), ld(s_taken + (idx >> 5)) | (int)(1u << (idx & 31)));
            }
            nm++;
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // the stores are done before the next point's loads
          }
        }
      }
#endif
      __syncthreads();
      q0 = q1;
    }

#ifndef ORBX_PROJMATCH_NO_HIST             // (a timing build without phase D: tools/projmatch_times.py)
    // ---- phase D: the rotation histogram (:1971-1981), its three maxima and the removal (:1988-2007); the Sim3 overloads have none
    if (g.check_ori && kind == 0) {        // uniform over the workgroup
      for (int q = tid; q < npts; q += kThreads) {
        const int i = res[q];
        if (i < 0 || i >= n) continue;
        const int bin = rot_bin(pts[q].angle, kp_field<float>(kp, i, kAngle));
        if (bin >= 0) atomicAdd(&s_hist[bin], 1);
        res[q] = i | (bin + 1) << 16;      // i < 32768; bin + 1 in 0 .. 30
      }
      __syncthreads();
      if (tid == 0) {                      // ComputeThreeMaxima, src/ORBmatcher.cc:2012-2053
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
      for (int q = tid; q < npts; q += kThreads) {
        const int r = res[q];
        if (r < 0) continue;
        const int bin = (r >> 16) - 1, i = r & 0xFFFF;   // i < n: only such results were given a bin
        if (bin < 0 || bin == ind1 || bin == ind2 || bin == ind3) continue;
        omatch[i] = -2;                    // after the chain's store to the same word: the workgroup's barriers lie between them
        atomicAdd(&s_removed, 1);
      }
      __syncthreads();
    }
#endif
    if (tid == 0) g.nmatches[b] = nm - s_removed;
  }
}

}  // namespace

struct orbx_projmatch : orbx::side::Handle {   // scratch: per workgroup the global path's arrays
  int lds_limit = kLdsMax;                     // ORBX_PROJMATCH_LDS at create
};

namespace {

using namespace orbx::side;

const char* side_problem(const orbx_projmatch_side* s) {
  if (!s) return "null side";
  if (s->nframes < 1 || s->capacity < 1) return "nframes and capacity must be at least 1";
  if (s->capacity > kMaxCap) return "capacity above 32768";
  if (!s->d_kps || !s->d_desc || !s->d_counts || !s->d_bounds) return "null buffer in the side";
  if ((long long)s->nframes * s->capacity > (long long)INT_MAX) return "nframes * capacity exceeds INT_MAX";
  return nullptr;
}

// what both forms check before anything is copied or launched
int check_call(orbx_projmatch* m, const char* who, const orbx_projmatch_side* side, const void* items, int nitems, const void* points,
               const void* npts, int mcap, const void* pdesc, int npoints, const float* sf, int nlevels, const void* kp_match,
               const void* nmatches) {
  if (const char* e = side_problem(side)) return fail(m, ORBX_E_INVALID, std::string(who) + e);
  if (!items || !points || !npts || !pdesc) return fail(m, ORBX_E_INVALID, std::string(who) + "null items, points, npts or pdesc");
  if (!kp_match || !nmatches) return fail(m, ORBX_E_INVALID, std::string(who) + "null kp_match or nmatches");
  if (nitems < 1 || mcap < 1 || npoints < 1) return fail(m, ORBX_E_INVALID, std::string(who) + "nitems, mcap and npoints must be at least 1");
  if (!sf || nlevels < 1 || nlevels > ORBX_PROJMATCH_MAX_LEVELS)
    return fail(m, ORBX_E_INVALID, std::string(who) + "scale_factors and nlevels in 1 .. 16 are needed (nlevels = " + std::to_string(nlevels) + ")");
  if ((long long)mcap * side->capacity > (long long)INT_MAX || (long long)nitems * std::max(mcap, side->capacity) > (long long)INT_MAX)
    return fail(m, ORBX_E_INVALID, std::string(who) + "mcap * capacity or nitems * max(mcap, capacity) exceeds INT_MAX");
  return ORBX_OK;
}

}  // namespace

extern "C" {

int orbx_projmatch_create(orbx_projmatch** out, int device) {
  return create_handle(out, device, "orbx_projmatch_create", orbx_projmatch_destroy, [](orbx_projmatch* m) {
    m->lds_limit = env_int("ORBX_PROJMATCH_LDS", 0, kLdsMax, kLdsMax);
    return allow_lds((const void*)k_proj_match<true>, kLdsMax);
  });
}

void orbx_projmatch_destroy(orbx_projmatch* m) { destroy_handle(m); }

const char* orbx_projmatch_last_error(const orbx_projmatch* m) { return last_error(m); }

int orbx_projmatch_search_device(orbx_projmatch* m, const orbx_projmatch_side* side, const orbx_projmatch_item* d_items, int nitems,
                                 const orbx_projmatch_point* d_points, const int32_t* d_npts, int mcap, const uint8_t* d_pdesc, int npoints,
                                 const float* scale_factors, int nlevels, int check_orientation, const uint8_t* d_kp_taken,
                                 int32_t* d_kp_match, int32_t* d_nmatches, void* stream) {
  if (!m) return ORBX_E_INVALID;
  const char* who = "orbx_projmatch_search_device: ";
  int rc = check_call(m, who, side, d_items, nitems, d_points, d_npts, mcap, d_pdesc, npoints, scale_factors, nlevels, d_kp_match, d_nmatches);
  if (rc != ORBX_OK) return rc;
  if (((uintptr_t)side->d_desc | (uintptr_t)d_points | (uintptr_t)d_pdesc) & 15)
    return fail(m, ORBX_E_INVALID, std::string(who) + "d_desc, d_points and d_pdesc must be 16-byte aligned");
  rc = same_device(m, who, {side->d_kps, side->d_desc, side->d_counts, side->d_bounds, d_items, d_points, d_npts, d_pdesc, d_kp_taken,
                            d_kp_match, d_nmatches}, "the handle");
  if (rc != ORBX_OK) return rc;
  ORBX_SIDE_HIP(m, hipSetDevice(m->device));
  const int cap = side->capacity;
  int p2 = 2;
  while (p2 < cap) p2 <<= 1;
  Paths path;                              // one point's longest list is cap candidates
  if ((rc = plan_paths(m, m->lds_limit, layout(cap, mcap, p2, true).fixed, layout(cap, mcap, p2, false).fixed, cap, nitems,
                       {kMaxBlocks, kGlobalBlocks, kGlobalRoom}, &path)) != ORBX_OK) return rc;
  Args g;
  g.kps = (const uint8_t*)side->d_kps; g.desc = side->d_desc; g.counts = side->d_counts; g.bounds = side->d_bounds;
  g.items = d_items; g.pts = d_points; g.npts = d_npts; g.pdesc = d_pdesc;
  g.kp_taken = d_kp_taken; g.kp_match = d_kp_match; g.nmatches = d_nmatches;
  g.scratch = path.in_lds ? nullptr : m->scratch.p; g.scratch_stride = path.scratch_stride;
  g.nframes = side->nframes; g.cap = cap; g.nitems = nitems; g.mcap = mcap; g.npoints = npoints; g.nlevels = nlevels; g.p2 = p2; g.room = path.room;
  g.check_ori = check_orientation != 0;
  for (int l = 0; l < ORBX_PROJMATCH_MAX_LEVELS; l++) g.sf[l] = l < nlevels ? scale_factors[l] : 0.0f;
  hipStream_t st = stream ? (hipStream_t)stream : m->st;
  if ((rc = wait_previous(m, st)) != ORBX_OK) return rc;
  if (path.in_lds) hipLaunchKernelGGL(k_proj_match<true>, dim3((unsigned)path.blocks), dim3(kThreads), path.lds_bytes, st, g);
  else hipLaunchKernelGGL(k_proj_match<false>, dim3((unsigned)path.blocks), dim3(kThreads), 0, st, g);
  return record_call(m, st);
}

int orbx_projmatch_search(orbx_projmatch* m, const orbx_projmatch_side* side, const orbx_projmatch_item* items, int nitems,
                          const orbx_projmatch_point* points, const int32_t* npts, int mcap, const uint8_t* pdesc, int npoints,
                          const float* scale_factors, int nlevels, int check_orientation, const uint8_t* kp_taken, int32_t* kp_match,
                          int32_t* nmatches) {
  if (!m) return ORBX_E_INVALID;
  const char* who = "orbx_projmatch_search: ";
  int rc = check_call(m, who, side, items, nitems, points, npts, mcap, pdesc, npoints, scale_factors, nlevels, kp_match, nmatches);
  if (rc != ORBX_OK) return rc;
  Stager io;
  const size_t nf = (size_t)side->nframes, nk = nf * side->capacity, rows = (size_t)nitems * side->capacity;
  const size_t o_kps = io.in(side->d_kps, nk * sizeof(orbx_keypoint)), o_desc = io.in(side->d_desc, nk * 32), o_counts = io.in(side->d_counts, nf * 8);
  const size_t o_bounds = io.in(side->d_bounds, nf * 16);
  const size_t o_items = io.in(items, (size_t)nitems * sizeof(orbx_projmatch_item));
  const size_t o_pts = io.in(points, (size_t)nitems * mcap * sizeof(orbx_projmatch_point));
  const size_t o_npts = io.in(npts, (size_t)nitems * 4), o_pdesc = io.in(pdesc, (size_t)npoints * 32);
  const size_t o_taken = kp_taken ? io.in(kp_taken, rows) : 0;
  const size_t o_match = io.out(kp_match, rows * 4), o_nm = io.out(nmatches, (size_t)nitems * 4);
  if ((rc = upload(m, io)) != ORBX_OK) return rc;
  uint8_t* const d = m->io.p;
  const orbx_projmatch_side ds = {(const orbx_keypoint*)(d + o_kps), d + o_desc, (const int32_t*)(d + o_counts), (const float*)(d + o_bounds),
                                  side->nframes, side->capacity};
  rc = orbx_projmatch_search_device(m, &ds, (const orbx_projmatch_item*)(d + o_items), nitems, (const orbx_projmatch_point*)(d + o_pts),
                                    (const int32_t*)(d + o_npts), mcap, d + o_pdesc, npoints, scale_factors, nlevels, check_orientation,
                                    kp_taken ? d + o_taken : nullptr, (int32_t*)(d + o_match), (int32_t*)(d + o_nm), m->st);
  if (rc != ORBX_OK) return rc;
  return download(m, io);
}

}  // extern "C"
