// The batched frame-to-last-frame matcher (include/orbx_lastmatch.h): ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame&
// LastFrame, th, bMono) (src/ORBmatcher.cc:1676-1885, Nleft == -1) for B (current frame, last frame's points) items on the keypoints and
// descriptors a batch extraction left in HBM and the points' descriptors in the pool ComputeDistinctiveDescriptors fills.
//
// k_last_match<LDS>: one workgroup of 8 waves per item (a grid of at most kMaxBlocks workgroups walks the items); the shape is
// csrc/localmatch/orbx_localmatch.hip's, written out again here (its pieces do not move without changing that kernel's assembly).
//   check, all waves     the item's frame, count, nlast, direction and th and every valid point's octave and pool row, before any of them
//                        addresses memory.
//   phase A, all waves   the frame's keypoints as keys (cell << 16 | index), sorted (bitonic, keys are unique: the order is the frame grid's:
//                        cells x-major, then y, then ascending index), a 16-byte record {x, y, octave, uright} per sorted position, the cells'
//                        starts by binary search.  A LANE PER POINT walks its window twice: once to count, and after a workgroup scan, for a
//                        chunk of points whose lists fit the candidate room, once to write its list with the point's descriptor in 8
//                        registers.  A candidate is one word: index (15 bits), Hamming distance (9).  The level range of the item's
//                        direction, the strict window test and the stereo gate are applied here; the kp_obs test is the chain's.  (Only a
//                        best is kept, so entries above 100 could be left out of the lists; they are not: leaving them out would need the
//                        distances in the counting walk too, and the chain passes over them in the same trip.)
//   phase B, wave 0      the chain over the chunk's points in index order: lane j holds candidate j (+ 64 per trip), drops the entries whose
//                        keypoint is hidden (a bit per keypoint in LDS, from the kp_obs row, set on every acceptance with obs > 0), keeps its
//                        smallest (distance << 15 | position) key; one DPP min-reduction gives the wave's smallest: the first in walk order
//                        among equal distances.  The accept test is wave-uniform; one lane records the point's keypoint and sets the hidden
//                        bit.  No descriptor and no keypoint is read here.  A and B repeat per chunk: the distances do not depend on the
//                        chain, so where the chunks are cut changes nothing.
//   phase C, all waves   kp_match[keypoint] = the LAST accepted point that took it (an integer maximum over the points' indices), then
//                        kp_obs[keypoint] = that point's obs.
//   phase D, all waves   under check_orientation: every accepted point's bin (integer adds into 30 LDS counters), ComputeThreeMaxima by one
//                        lane, then every entry of another bin writes kp_match = -2, kp_obs = -1 and counts itself (an integer add): entries
//                        of one keypoint write the same values, so nothing depends on the order.
// LDS path: the frame's descriptors (16-byte LDS-DMA loads), the grid, the offsets, the points' results and the candidate room in LDS.
// Global path (sizes that need more LDS than the handle's limit): the descriptors where they lie, everything else in the workgroup's slice of
// the handle's scratch.  The hidden bits are 4 KiB of static LDS on both paths.
// The float expressions are compiled with -ffp-contract=off: every operation is rounded by itself, as the specification states them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>

#include "../side/orbx_handle.h"
#include "../side/orbx_pair_device.h"
#include "../../../include/orbx_lastmatch.h"

namespace {

using namespace orbx::side::dev;          // ld / st on the chain's state: written by one lane, read by the wave's other lanes in the next step

constexpr int kThreads = 512;             // 8 waves
constexpr int kLdsMax = 148 * 1024;       // dynamic LDS of one workgroup (160 KiB per CU, the static part is below 8 KiB)
constexpr int kMaxBlocks = 1024;          // workgroups of one launch on the LDS path
constexpr int kGlobalBlocks = 256;        // ... on the global path: each owns one slice of the scratch
constexpr int kGlobalRoom = 64 * 1024;    // candidates of one chunk on the global path (at least the capacity)
constexpr int kMaxCap = ORBX_LASTMATCH_MAX_CAPACITY;   // a key and a candidate hold a 15-bit index
constexpr int kCols = 64, kRows = 48, kCells = kCols * kRows;
constexpr int kThHigh = 100, kBins = 30;
constexpr int kNone = INT_MAX;            // no key
static_assert(kMaxCap == 32768, "15-bit indices and positions");

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
  const uint8_t* kps; const uint8_t* desc; const int32_t* counts; const float* uright; const float* bounds;
  const orbx_lastmatch_item* items; const orbx_lastmatch_point* pts; const int32_t* nlast; const uint8_t* pdesc;
  int32_t* kp_obs; int32_t* kp_match; int32_t* nmatches;
  uint8_t* scratch; size_t scratch_stride;
  int nframes, cap, nitems, mcap, npoints, nlevels, p2, room, check_ori;
  float sf[ORBX_LASTMATCH_MAX_LEVELS];
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

// Frame::GetFeaturesInArea(x, y, r, minLevel, maxLevel) (src/Frame.cc:657-723) over the sorted records: emit(record, index) for every
// candidate, in the reference's order.
template <class F>
__device__ __forceinline__ void walk(float minX, float minY, float invW, float invH, float x, float y, float r, int minLevel, int maxLevel,
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
  const bool levels = minLevel > 0 || maxLevel >= 0;   // bCheckLevels
  for (int ix = x0; ix <= x1; ix++) {      // the cells (ix, y0 .. y1) are neighbours in the sorted keys
    const int j1 = cstart[ix * kRows + y1 + 1];
    for (int j = cstart[ix * kRows + y0]; j < j1; j++) {
      const Rec c = recs[j];
      if (levels) {
        if (c.octave < minLevel) continue;
        if (maxLevel >= 0 && c.octave > maxLevel) continue;
      }
      if (fabsf(c.x - x) < r && fabsf(c.y - y) < r) emit(c, (int)(keys[j] & 0xFFFFu));
    }
  }
}

// a point's window: th times the octave's scale (:1724), the direction's level range (:1728-1733), the right coordinate of the gate (:1753)
struct Pt { float x, y, xr, radius; int lo, hi, point; bool live; };
__device__ __forceinline__ Pt load_point(const orbx_lastmatch_point* p, const float* s_sf, float th, float mbf, int direction) {
  const uint4* const rp = (const uint4*)p;
  const uint4 lo = rp[0], hi = rp[1];
  Pt t;
  t.x = __uint_as_float(lo.x); t.y = __uint_as_float(lo.y);
  const float invz = __uint_as_float(lo.z);
  const int octave = (int)hi.x;
  t.point = (int)hi.z;
  // valid, and finite: a NaN fails every comparison (the reference leaves a non-finite projection undefined; here it has no candidate)
  t.live = hi.w != 0u && fabsf(t.x) < INFINITY && fabsf(t.y) < INFINITY;
  t.radius = 0.0f; t.xr = 0.0f; t.lo = 0; t.hi = 0;
  if (t.live) {                            // the octave is one of the table's: the check
    t.radius = th * s_sf[octave];
    {
#pragma clang fp contract(off)             // a product rounded to float32, then a subtraction: an FMA here changes results
      const float prod = mbf * invz;
      t.xr = t.x - prod;
    }
    if (direction == 1) { t.lo = octave; t.hi = -1; }
    else if (direction == 2) { t.lo = 0; t.hi = octave; }
    else { t.lo = octave - 1; t.hi = octave + 1; }
  }
  return t;
}

template <bool LDS>
__global__ __launch_bounds__(kThreads) void k_last_match(Args g) {
  extern __shared__ __align__(16) uint8_t smem[];
  __shared__ int s_cnt, s_bad, s_removed;
  __shared__ int s_hist[32], s_ind[3];
  __shared__ int s_scan[kThreads];
  __shared__ int32_t s_hidden[kMaxCap / 32];   // bit i: keypoint i holds a map point with Observations() > 0
  __shared__ float s_sf[ORBX_LASTMATCH_MAX_LEVELS];
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

  if (tid < ORBX_LASTMATCH_MAX_LEVELS) {   // the level table: constant indices into the kernel's arguments
    float v = 0.0f;
#pragma unroll
    for (int l = 0; l < ORBX_LASTMATCH_MAX_LEVELS; l++)
      if (tid == l) v = g.sf[l];
    s_sf[tid] = v;
  }

  for (int b = blockIdx.x; b < g.nitems; b += gridDim.x) {
    __syncthreads();                       // the previous item's shared state has been read
    int32_t* const omatch = g.kp_match + (size_t)b * cap;
    int32_t* const oobs = g.kp_obs + (size_t)b * cap;
    const orbx_lastmatch_point* const pts = g.pts + (size_t)b * mcap;
    // ---- the check: nothing below addresses memory with a value that was not tested here
    const int f = g.items[b].frame, direction = g.items[b].direction, nlast = g.nlast[b];
    const float mbf = g.items[b].mbf, th = g.items[b].th;
    bool ok = f >= 0 && f < g.nframes && nlast >= 0 && nlast <= mcap && direction >= 0 && direction <= 2 && fabsf(th) < INFINITY;
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
      for (int q = tid; q < nlast; q += kThreads) {
        const uint4 hi = ((const uint4*)(pts + q))[1];
        bad |= hi.w != 0u && ((int)hi.x < 0 || (int)hi.x >= g.nlevels || (int)hi.z < 0 || (int)hi.z >= g.npoints);
      }
      if (bad) s_bad = 1;
    }
    __syncthreads();
    if (!ok || s_bad) {                    // uniform over the workgroup: a row of -1, kp_obs as it was
      if (tid == 0) g.nmatches[b] = -1;
      continue;
    }
    const size_t of = (size_t)f * cap;
    const uint8_t* const kp = g.kps + of * sizeof(orbx_keypoint);
    const float* const ur = g.uright ? g.uright + of : nullptr;
    const uint8_t* const desc = LDS ? base + L.desc : g.desc + of * 32;
    const float minX = g.bounds[4 * f], minY = g.bounds[4 * f + 1];
    const float invW = div_rn((float)kCols, g.bounds[4 * f + 2] - minX), invH = div_rn((float)kRows, g.bounds[4 * f + 3] - minY);   // src/Frame.cc:153-160

    // ---- phase A: the frame's grid
    if (LDS) stage_dma<kThreads>(base + L.desc, g.desc + of * 32, n * 2);
    for (int w = tid; w < kMaxCap / 32; w += kThreads) s_hidden[w] = 0;
    for (int q = tid; q < nlast; q += kThreads) res[q] = -1;
    __syncthreads();
    for (int i = tid; i < n; i += kThreads) {
      if (oobs[i] > 0) atomicOr(&s_hidden[i >> 5], (int)(1u << (i & 31)));
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
      recs[j] = Rec{kp_field<float>(kp, i, kX), kp_field<float>(kp, i, kY), kp_field<int32_t>(kp, i, kOctave), ur ? ur[i] : -1.0f};
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
    for (int q = tid; q <= nlast; q += kThreads) {
      int c = 0;
      if (q < nlast) {
        const Pt t = load_point(pts + q, s_sf, th, mbf, direction);
        if (t.live)
          walk(minX, minY, invW, invH, t.x, t.y, t.radius, t.lo, t.hi, cstart, recs, keys, [&](const Rec& r, int) {
            if (r.ur > 0.0f && fabsf(t.xr - r.ur) > t.radius) return;   // the stereo gate, src/ORBmatcher.cc:1751-1757
            c++;
          });
      }
      offs[q] = c;
    }
    __syncthreads();
    {
      const int m = nlast + 1, per = (m + kThreads - 1) / kThreads;
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
    for (int q0 = 0; q0 < nlast;) {
      const int e0 = offs[q0];
      int q1;
      {                                    // the largest q1 with offs[q1] - e0 <= room; one point's list (<= cap <= room) always fits
        int lo = q0 + 1, hi = nlast;
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
          const Pt t = load_point(pts + q, s_sf, th, mbf, direction);
          const D8 qd = load_desc(g.pdesc + (size_t)t.point * 32);   // the pool row is below npoints: the check
          walk(minX, minY, invW, invH, t.x, t.y, t.radius, t.lo, t.hi, cstart, recs, keys, [&](const Rec& r, int i) {
            if (r.ur > 0.0f && fabsf(t.xr - r.ur) > t.radius) return;
            if (k < kend && k < tot) {
              const int d = hamming(qd, load_desc(desc + (size_t)i * 32));
              cand[k] = (uint32_t)i | (uint32_t)d << 15;
            }
            k++;
          });
        }
      }
      __syncthreads();

#ifndef ORBX_LASTMATCH_NO_CHAIN            // (a timing build without phase B: tools/lastmatch_times.py; its results are not the specification's)
      if (tid < 64) {                      // ---- phase B
        for (int c0 = q0; c0 < q1; c0 += 64) {
          const int cn = min(64, q1 - c0);
          int l_b = 0, l_n = 0, l_obs = 0;
          if (lane < cn) {
            l_b = offs[c0 + lane] - e0; l_n = offs[c0 + lane + 1] - e0 - l_b;
            l_obs = pts[c0 + lane].obs;
          }
          for (int i = 0; i < cn; i++) {
            const int cnt = __builtin_amdgcn_readlane(l_n, i);
            if (cnt <= 0) continue;
            const int b0 = __builtin_amdgcn_readlane(l_b, i);
            int k1 = kNone;                // the lane's smallest (distance << 15 | position)
            for (int j = lane; j < cnt; j += 64) {
              const uint32_t e = cand[b0 + j];
              const int idx = (int)(e & 0x7FFFu);
              if ((ld(s_hidden + (idx >> 5)) >> (idx & 31)) & 1) continue;
              k1 = min(k1, (int)((e >> 15) & 0x1FFu) << 15 | j);
            }
            const int m1 = wave_min(k1);
            if (m1 == kNone || (m1 >> 15) > kThHigh) continue;   // :1770
            const int obs = __builtin_amdgcn_readlane(l_obs, i);
            if (lane == 0) {
              const int idx = (int)(cand[b0 + (m1 & 0x7FFF)] & 0x7FFFu);
              st(res + c0 + i, idx);
              if (obs > 0) st(s_hidden + (idx >> 5), ld(s_hidden + (idx >> 5)) | (int)(1u << (idx & 31)));
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

    // ---- phase C: the last point that took a keypoint holds it; integer maxima, so the order does not matter
    for (int q = tid; q < nlast; q += kThreads) {
      const int i = res[q];
      if (i >= 0 && i < n) __hip_atomic_fetch_max(omatch + i, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    for (int i = tid; i < n; i += kThreads) {
      const int q = __hip_atomic_load(omatch + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (q >= 0 && q < nlast) oobs[i] = pts[q].obs;
    }
#ifndef ORBX_LASTMATCH_NO_HIST             // (a timing build without phase D: tools/lastmatch_times.py)
    // ---- phase D: the rotation histogram (:1775-1792), its three maxima and the removal (:1862-1882)
    if (g.check_ori) {                     // uniform over the grid
      for (int q = tid; q < nlast; q += kThreads) {
        const int i = res[q];
        if (i < 0 || i >= n) continue;
        const int bin = rot_bin(pts[q].angle, kp_field<float>(kp, i, kAngle));
        if (bin >= 0) atomicAdd(&s_hist[bin], 1);
        res[q] = i | (bin + 1) << 16;      // i < 32768; bin + 1 in 0 .. 30
      }
      __syncthreads();                     // phase C's reads of kp_match and writes of kp_obs are done as well
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
      for (int q = tid; q < nlast; q += kThreads) {
        const int r = res[q];
        if (r < 0) continue;
        const int bin = (r >> 16) - 1, i = r & 0xFFFF;   // i < n: only such results were given a bin
        if (bin < 0 || bin == ind1 || bin == ind2 || bin == ind3) continue;
        omatch[i] = -2; oobs[i] = -1;
        atomicAdd(&s_removed, 1);
      }
      __syncthreads();
    }
#endif
    if (tid == 0) g.nmatches[b] = nm - s_removed;
  }
}

}  // namespace

struct orbx_lastmatch : orbx::side::Handle {   // scratch: per workgroup the global path's arrays
  int lds_limit = kLdsMax;                     // ORBX_LASTMATCH_LDS at create
};

namespace {

using namespace orbx::side;

const char* side_problem(const orbx_lastmatch_side* s) {
  if (!s) return "null side";
  if (s->nframes < 1 || s->capacity < 1) return "nframes and capacity must be at least 1";
  if (s->capacity > kMaxCap) return "capacity above 32768";
  if (!s->d_kps || !s->d_desc || !s->d_counts || !s->d_bounds) return "null buffer in the side";
  if ((long long)s->nframes * s->capacity > (long long)INT_MAX) return "nframes * capacity exceeds INT_MAX";
  return nullptr;
}

// what both forms check before anything is copied or launched
int check_call(orbx_lastmatch* m, const char* who, const orbx_lastmatch_side* side, const void* items, int nitems, const void* points,
               const void* nlast, int mcap, const void* pdesc, int npoints, const float* sf, int nlevels, const void* kp_obs,
               const void* kp_match, const void* nmatches) {
  if (const char* e = side_problem(side)) return fail(m, ORBX_E_INVALID, std::string(who) + e);
  if (!items || !points || !nlast || !pdesc) return fail(m, ORBX_E_INVALID, std::string(who) + "null items, points, nlast or pdesc");
  if (!kp_obs || !kp_match || !nmatches) return fail(m, ORBX_E_INVALID, std::string(who) + "null kp_obs, kp_match or nmatches");
  if (nitems < 1 || mcap < 1 || npoints < 1) return fail(m, ORBX_E_INVALID, std::string(who) + "nitems, mcap and npoints must be at least 1");
  if (!sf || nlevels < 1 || nlevels > ORBX_LASTMATCH_MAX_LEVELS)
    return fail(m, ORBX_E_INVALID, std::string(who) + "scale_factors and nlevels in 1 .. 16 are needed (nlevels = " + std::to_string(nlevels) + ")");
  if ((long long)mcap * side->capacity > (long long)INT_MAX || (long long)nitems * std::max(mcap, side->capacity) > (long long)INT_MAX)
    return fail(m, ORBX_E_INVALID, std::string(who) + "mcap * capacity or nitems * max(mcap, capacity) exceeds INT_MAX");
  return ORBX_OK;
}

}  // namespace

extern "C" {

int orbx_lastmatch_create(orbx_lastmatch** out, int device) {
  return create_handle(out, device, "orbx_lastmatch_create", orbx_lastmatch_destroy, [](orbx_lastmatch* m) {
    m->lds_limit = env_int("ORBX_LASTMATCH_LDS", 0, kLdsMax, kLdsMax);
    return allow_lds((const void*)k_last_match<true>, kLdsMax);
  });
}

void orbx_lastmatch_destroy(orbx_lastmatch* m) { destroy_handle(m); }

const char* orbx_lastmatch_last_error(const orbx_lastmatch* m) { return last_error(m); }

int orbx_lastmatch_search_device(orbx_lastmatch* m, const orbx_lastmatch_side* side, const orbx_lastmatch_item* d_items, int nitems,
                                 const orbx_lastmatch_point* d_points, const int32_t* d_nlast, int mcap, const uint8_t* d_pdesc, int npoints,
                                 const float* scale_factors, int nlevels, int check_orientation, int32_t* d_kp_obs, int32_t* d_kp_match,
                                 int32_t* d_nmatches, void* stream) {
  if (!m) return ORBX_E_INVALID;
  const char* who = "orbx_lastmatch_search_device: ";
  int rc = check_call(m, who, side, d_items, nitems, d_points, d_nlast, mcap, d_pdesc, npoints, scale_factors, nlevels, d_kp_obs, d_kp_match,
                      d_nmatches);
  if (rc != ORBX_OK) return rc;
  if (((uintptr_t)side->d_desc | (uintptr_t)d_points | (uintptr_t)d_pdesc) & 15)
    return fail(m, ORBX_E_INVALID, std::string(who) + "d_desc, d_points and d_pdesc must be 16-byte aligned");
  rc = same_device(m, who, {side->d_kps, side->d_desc, side->d_counts, side->d_uright, side->d_bounds, d_items, d_points, d_nlast, d_pdesc,
                            d_kp_obs, d_kp_match, d_nmatches}, "the handle");
  if (rc != ORBX_OK) return rc;
  ORBX_SIDE_HIP(m, hipSetDevice(m->device));
  const int cap = side->capacity;
  int p2 = 2;
  while (p2 < cap) p2 <<= 1;
  Paths path;                              // one point's longest list is cap candidates
  if ((rc = plan_paths(m, m->lds_limit, layout(cap, mcap, p2, true).fixed, layout(cap, mcap, p2, false).fixed, cap, nitems,
                       {kMaxBlocks, kGlobalBlocks, kGlobalRoom}, &path)) != ORBX_OK) return rc;
  Args g;
  g.kps = (const uint8_t*)side->d_kps; g.desc = side->d_desc; g.counts = side->d_counts; g.uright = side->d_uright; g.bounds = side->d_bounds;
  g.items = d_items; g.pts = d_points; g.nlast = d_nlast; g.pdesc = d_pdesc;
  g.kp_obs = d_kp_obs; g.kp_match = d_kp_match; g.nmatches = d_nmatches;
  g.scratch = path.in_lds ? nullptr : m->scratch.p; g.scratch_stride = path.scratch_stride;
  g.nframes = side->nframes; g.cap = cap; g.nitems = nitems; g.mcap = mcap; g.npoints = npoints; g.nlevels = nlevels; g.p2 = p2; g.room = path.room;
  g.check_ori = check_orientation != 0;
  for (int l = 0; l < ORBX_LASTMATCH_MAX_LEVELS; l++) g.sf[l] = l < nlevels ? scale_factors[l] : 0.0f;
  hipStream_t st = stream ? (hipStream_t)stream : m->st;
  if ((rc = wait_previous(m, st)) != ORBX_OK) return rc;
  if (path.in_lds) hipLaunchKernelGGL(k_last_match<true>, dim3((unsigned)path.blocks), dim3(kThreads), path.lds_bytes, st, g);
  else hipLaunchKernelGGL(k_last_match<false>, dim3((unsigned)path.blocks), dim3(kThreads), 0, st, g);
  return record_call(m, st);
}

int orbx_lastmatch_search(orbx_lastmatch* m, const orbx_lastmatch_side* side, const orbx_lastmatch_item* items, int nitems,
                          const orbx_lastmatch_point* points, const int32_t* nlast, int mcap, const uint8_t* pdesc, int npoints,
                          const float* scale_factors, int nlevels, int check_orientation, int32_t* kp_obs, int32_t* kp_match,
                          int32_t* nmatches) {
  if (!m) return ORBX_E_INVALID;
  const char* who = "orbx_lastmatch_search: ";
  int rc = check_call(m, who, side, items, nitems, points, nlast, mcap, pdesc, npoints, scale_factors, nlevels, kp_obs, kp_match, nmatches);
  if (rc != ORBX_OK) return rc;
  Stager io;
  const size_t nf = (size_t)side->nframes, nk = nf * side->capacity, rows = (size_t)nitems * side->capacity;
  const size_t o_kps = io.in(side->d_kps, nk * sizeof(orbx_keypoint)), o_desc = io.in(side->d_desc, nk * 32), o_counts = io.in(side->d_counts, nf * 8);
  const size_t o_ur = side->d_uright ? io.in(side->d_uright, nk * 4) : 0, o_bounds = io.in(side->d_bounds, nf * 16);
  const size_t o_items = io.in(items, (size_t)nitems * sizeof(orbx_lastmatch_item));
  const size_t o_pts = io.in(points, (size_t)nitems * mcap * sizeof(orbx_lastmatch_point));
  const size_t o_nlast = io.in(nlast, (size_t)nitems * 4), o_pdesc = io.in(pdesc, (size_t)npoints * 32);
  const size_t o_obs = io.out(kp_obs, rows * 4, true), o_match = io.out(kp_match, rows * 4), o_nm = io.out(nmatches, (size_t)nitems * 4);
  if ((rc = upload(m, io)) != ORBX_OK) return rc;
  uint8_t* const d = m->io.p;
  const orbx_lastmatch_side ds = {(const orbx_keypoint*)(d + o_kps), d + o_desc, (const int32_t*)(d + o_counts),
                                  side->d_uright ? (const float*)(d + o_ur) : nullptr, (const float*)(d + o_bounds), side->nframes, side->capacity};
  rc = orbx_lastmatch_search_device(m, &ds, (const orbx_lastmatch_item*)(d + o_items), nitems, (const orbx_lastmatch_point*)(d + o_pts),
                                    (const int32_t*)(d + o_nlast), mcap, d + o_pdesc, npoints, scale_factors, nlevels, check_orientation,
                                    (int32_t*)(d + o_obs), (int32_t*)(d + o_match), (int32_t*)(d + o_nm), m->st);
  if (rc != ORBX_OK) return rc;
  return download(m, io);
}

}  // extern "C"
