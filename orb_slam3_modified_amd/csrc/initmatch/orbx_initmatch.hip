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
#include <cstring>
#include <string>

#include "../side/orbx_handle.h"
#include "../side/orbx_pair_device.h"
#include "../side/orbx_pair_host.h"
#include "../../../include/orbx_initmatch.h"

namespace {

using namespace orbx::side::dev;          // ld / st on the chain's state: written by one lane, read by the wave's other lanes in the next step

constexpr int kThreads = 512;             // 8 waves
constexpr int kGlobalBlocks = 256;        // workgroups of one launch on the global path (kMaxBlocks on the LDS path): each owns one slice of the scratch
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

constexpr size_t kX = offsetof(orbx_keypoint, x), kY = offsetof(orbx_keypoint, y), kAngle = offsetof(orbx_keypoint, angle),
                 kOctave = offsetof(orbx_keypoint, octave);

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
      stage_dma<kThreads>(base + L.dA, g.a.desc + oA * 32, nA * 2);
      stage_dma<kThreads>(base + L.dB, g.b.desc + oB * 32, nB * 2);
    }
    for (int i = tid; i < nB; i += kThreads) { mdist[i] = INT_MAX; holder[i] = -1; }
    for (int i = tid; i < nA; i += kThreads) { m12[i] = -1; acc[i] = -1; }
    __syncthreads();                       // s_cnt = 0 before anyone adds to it
    for (int i = tid; i < nB; i += kThreads) {
      if (kp_field<int32_t>(kB, i, kOctave) != 0) continue;
      const float fx = roundf((kp_field<float>(kB, i, kX) - g.minX) * g.invW), fy = roundf((kp_field<float>(kB, i, kY) - g.minY) * g.invH);
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
      sxy[j] = make_float2(kp_field<float>(kB, i, kX), kp_field<float>(kB, i, kY));
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
      if (q < nA && kp_field<int32_t>(kA, q, kOctave) == 0) {
        const float cx = prev ? prev[2 * q] : kp_field<float>(kA, q, kX), cy = prev ? prev[2 * q + 1] : kp_field<float>(kA, q, kY);
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
          const float cx = prev ? prev[2 * q] : kp_field<float>(kA, q, kX), cy = prev ? prev[2 * q + 1] : kp_field<float>(kA, q, kY);
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
              if (ld(mdist + i2) <= d) continue;
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
                const int was = ld(holder + ibest);
                if (was >= 0) st(m12 + was, -1);
                st(m12 + q, ibest);
                st(acc + q, ibest);
                st(holder + ibest, q);
                st(mdist + ibest, m);
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
          const int bin = rot_bin(kp_field<float>(kA, q, kAngle), kp_field<float>(kB, v, kAngle));
          if (bin >= 0) atomicAdd(&s_hist[bin], 1);
        }
      }
      __syncthreads();
      if (tid == 0) three_maxima(s_hist, s_ind);
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
          const int bin = rot_bin(kp_field<float>(kA, q, kAngle), kp_field<float>(kB, v, kAngle));
          if (bin >= 0 && bin != i1 && bin != i2 && bin != i3) v = -1;
        }
        if (v < 0 || v >= nB) v = -1;
      }
      o12[q] = v;
      if (v >= 0) {
        if (o21) o21[v] = q;
        if (prev) { prev[2 * q] = kp_field<float>(kB, v, kX); prev[2 * q + 1] = kp_field<float>(kB, v, kY); }
        cnt++;
      }
    }
    if (cnt) atomicAdd(&s_nm, cnt);
    __syncthreads();
    if (tid == 0) g.nm[p] = s_nm;
  }
}

}  // namespace

struct orbx_initmatch : orbx::side::pair::PairHandle {};   // scratch: per workgroup the global path's arrays

namespace {

using namespace orbx::side;
using namespace orbx::side::pair;

// what both forms check before anything is copied or launched
int check_call(orbx_initmatch* m, const char* who, const orbx_initmatch_side* a, const orbx_initmatch_side* b, const void* pairs, int npairs,
               const float* bounds, int window, const void* m12, const void* nm) {
  int rc = check_sides<false>(m, who, a, b, kMaxCap, "capacity above 32768", pairs && m12 && nm && bounds, "pairs, bounds, matches12 or nmatches");
  if (rc != ORBX_OK || (rc = check_npairs(m, who, npairs)) != ORBX_OK) return rc;
  if (window < 0) return fail(m, ORBX_E_INVALID, std::string(who) + "window_size = " + std::to_string(window) + " (at least 0)");
  if (!(bounds[2] > bounds[0]) || !(bounds[3] > bounds[1])) return fail(m, ORBX_E_INVALID, std::string(who) + "bounds: max must be above min");
  return check_sizes<false>(m, who, a, b, npairs, 2LL * std::max(a->capacity, b->capacity), "npairs * capacity");
}

}  // namespace

extern "C" {

int orbx_initmatch_create(orbx_initmatch** out, int device) {
  return create_handle(out, device, "orbx_initmatch_create", orbx_initmatch_destroy, [](orbx_initmatch* m) {
    return open_pair(m, "ORBX_INITMATCH_LDS", nullptr, (const void*)k_init_pairs<true>);
  });
}

void orbx_initmatch_destroy(orbx_initmatch* m) { destroy_handle(m); }

const char* orbx_initmatch_last_error(const orbx_initmatch* m) { return last_error(m); }

int orbx_initmatch_pairs_device(orbx_initmatch* m, const orbx_initmatch_side* a, const orbx_initmatch_side* b, const int32_t* d_pairs, int npairs,
                                const float bounds[4], int window_size, float nn_ratio, int check_orientation, float* d_prev_xy,
                                int32_t* d_matches12, int32_t* d_matches21, int32_t* d_nmatches, void* stream) {
  if (!m) return ORBX_E_INVALID;
  const char* who = "orbx_initmatch_pairs_device: ";
  int rc = check_call(m, who, a, b, d_pairs, npairs, bounds, window_size, d_matches12, d_nmatches);
  if (rc != ORBX_OK) return rc;
  rc = same_device(m, who, {a->d_kps, a->d_desc, a->d_counts, b->d_kps, b->d_desc, b->d_counts, d_pairs, d_prev_xy, d_matches12, d_matches21, d_nmatches},
                   "the handle");
  if (rc != ORBX_OK) return rc;
  ORBX_SIDE_HIP(m, hipSetDevice(m->device));
  const int capA = a->capacity, capB = b->capacity;
  int p2 = 2;
  while (p2 < capB) p2 <<= 1;
  Paths path;                              // one query's longest list is capB candidates; the global path's scratch is grown here
  if ((rc = plan_paths(m, m->lds_limit, layout(capA, capB, p2, true).fixed, layout(capA, capB, p2, false).fixed, capB, npairs,
                       {kMaxBlocks, kGlobalBlocks, kGlobalRoom}, &path)) != ORBX_OK) return rc;
  Args g;
  g.a = {(const uint8_t*)a->d_kps, a->d_desc, a->d_counts, a->nframes, capA};
  g.b = {(const uint8_t*)b->d_kps, b->d_desc, b->d_counts, b->nframes, capB};
  g.pairs = d_pairs; g.prev = d_prev_xy; g.m12 = d_matches12; g.m21 = d_matches21; g.nm = d_nmatches;
  g.npairs = npairs; g.p2 = p2; g.room = path.room; g.check_ori = check_orientation != 0;
  g.minX = bounds[0]; g.minY = bounds[1];
  g.invW = (float)kCols / (bounds[2] - bounds[0]); g.invH = (float)kRows / (bounds[3] - bounds[1]);
  g.r = (float)window_size; g.ratio = nn_ratio;
  return launch(m, path.in_lds, path.lds_bytes, path.scratch_stride, path.blocks, kThreads, g, k_init_pairs<true>, k_init_pairs<false>, stream);
}

int orbx_initmatch_pairs(orbx_initmatch* m, const orbx_initmatch_side* a, const orbx_initmatch_side* b, const int32_t* pairs, int npairs,
                         const float bounds[4], int window_size, float nn_ratio, int check_orientation, float* prev_xy, int32_t* matches12,
                         int32_t* matches21, int32_t* nmatches) {
  if (!m) return ORBX_E_INVALID;
  const char* who = "orbx_initmatch_pairs: ";
  int rc = check_call(m, who, a, b, pairs, npairs, bounds, window_size, matches12, nmatches);
  if (rc != ORBX_OK) return rc;
  const auto arrays = side_arrays<false, orbx_initmatch_side>();
  Stager io;
  const StagedSides off = stage_sides(io, a, b, arrays);
  const size_t o_pairs = io.in(pairs, (size_t)npairs * 8);
  const size_t n12 = (size_t)npairs * a->capacity * 4, n21 = (size_t)npairs * b->capacity * 4, nprev = prev_xy ? n12 * 2 : 0;
  const size_t o_prev = io.out(prev_xy, nprev, true), o_12 = io.out(matches12, n12), o_21 = io.out(matches21, n21),
               o_nm = io.out(nmatches, (size_t)npairs * 4);
  if ((rc = upload(m, io)) != ORBX_OK) return rc;
  uint8_t* d = m->io.p;
  orbx_initmatch_side ds[2];
  device_sides(d, off, a, b, arrays, ds);
  rc = orbx_initmatch_pairs_device(m, &ds[0], &ds[1], (const int32_t*)(d + o_pairs), npairs, bounds, window_size, nn_ratio, check_orientation,
                                   prev_xy ? (float*)(d + o_prev) : nullptr, (int32_t*)(d + o_12), (int32_t*)(d + o_21), (int32_t*)(d + o_nm), m->st);
  if (rc != ORBX_OK) return rc;
  return download(m, io);
}

}  // extern "C"
