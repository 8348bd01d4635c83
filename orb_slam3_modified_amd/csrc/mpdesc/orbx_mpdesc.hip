// The batched MapPoint::ComputeDistinctiveDescriptors (include/orbx_mpdesc.h, src/MapPoint.cc:329-403): for M map points at once, of a
// point's N observed descriptors the one whose median Hamming distance to the others is least, on the descriptors a batch extraction left
// in HBM.  Four launches whatever the points are, no host synchronisation:
//
// k_mpd_classify: a thread per point.  obs_start, N and the out row are checked before any of them addresses memory; the point's class
//   {malformed, empty, small, mid, large} goes to the handle's memory, malformed and empty points get their result here, mid and large
//   points are appended to one index list each (an atomic counter: the lists' order varies, no result depends on it).
// k_mpd_small (N <= small_max <= 64): A LANE PER OBSERVATION.  Most points have 2 - 30 observations, which would leave a wave per point
//   idle.  A workgroup of 256 lanes owns 128 consecutive points: a scan of their N gives every small observation of the chunk a flat
//   index, and the chunk is walked in passes of 256 flat indices, so several points share a wave and a point may straddle waves and
//   passes.  First every observation's (frame, row) is checked; a bad one marks its point.  A pass stages the descriptors of every point
//   it touches in LDS (at most 256 + 2 * 63 of them), each lane walks its own point's N descriptors (8 x xor + popcount) and keeps its row
//   of distances in LDS as 16-bit values ([j][lane]: conflict-free), finds the row's k-th smallest without sorting -- a binary search on
//   the VALUE 0 .. 256, nine counts of `distance <= v` -- and the point's winner is an LDS min over the key (median << 11) | i: exactly
//   "strict <, the first i wins" because i < 2048.  A workgroup owns whole points, so nothing crosses workgroups.
// k_mpd_point<true> (N <= mid_max <= 256): a workgroup of 256 per point of the mid list, a lane per row, the N x N distances in LDS as
//   16-bit values (they reach 256; stored [j][lane], so a lane's row is a column of consecutive halfwords and needs no odd pitch).
// k_mpd_point<false> (N <= 1024): a workgroup of 1024 per point of the large list, the descriptors in LDS, every count of the binary
//   search recomputes the row's distances (a 1024 x 1024 matrix does not fit).
// Both walk their list with a grid stride: the list's length is known on the device only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <string>

#include "../side/orbx_handle.h"
#include "../side/orbx_pair_device.h"
#include "../../../include/orbx_mpdesc.h"

namespace {

using namespace orbx::side::dev;

constexpr int kSmallCap = 64;             // the largest N the lane-per-observation form can take
constexpr int kMidCap = 256;              // the largest N the matrix form can take: its workgroup's size
constexpr int kChunk = 128;               // points of one workgroup of k_mpd_small
constexpr int kLanes = 256;               // its lanes: the flat indices of one pass
constexpr int kStage = kLanes + 2 * kSmallCap;   // descriptors a pass stages: its own and those of the points that straddle its two ends
constexpr int kMidGrid = 512, kLargeGrid = 256;  // workgroups that walk the mid and the large list
constexpr int kMidLds = kMidCap * 32 + kMidCap * kMidCap * 2, kLargeLds = ORBX_MPDESC_MAX_OBS * 32;
static_assert(kChunk % 64 == 0 && kChunk <= kLanes && kStage >= kLanes + 2 * (kSmallCap - 1), "the scan's and the staging's shapes");
static_assert(ORBX_MPDESC_MAX_OBS < 2048 && kMidLds <= 155648, "the key's index field; the LDS block");

enum : int32_t { kBad = 0, kEmpty = 1, kSmall = 2, kMid = 3, kLarge = 4 };

struct Args {
  const uint8_t* desc; const int32_t* counts; const int2* obs; const int32_t* start; const int32_t* out_row; uint4* out_desc;
  int32_t* best; int32_t* median;
  int32_t* cls; int32_t* list_mid; int32_t* list_large; int32_t* cnt;   // cnt[0]: mid points, cnt[1]: large points
  int nframes, cap, nobs, npoints, out_rows, small_max, mid_max;
};

// an observation names a row the side holds
__device__ __forceinline__ bool obs_ok(const Args& g, int2 o) {
  if (o.x < 0 || o.x >= g.nframes || o.y < 0) return false;
  return o.y < min(g.counts[2 * o.x], g.cap);
}
// its descriptor; obs_ok(o) holds
__device__ __forceinline__ const uint4* desc_of(const Args& g, int2 o) { return (const uint4*)(g.desc + ((size_t)o.x * g.cap + o.y) * 32); }

__device__ __forceinline__ D8 d8(uint4 x, uint4 y) {
  D8 d;
  d.w[0] = x.x; d.w[1] = x.y; d.w[2] = x.z; d.w[3] = x.w; d.w[4] = y.x; d.w[5] = y.y; d.w[6] = y.z; d.w[7] = y.w;
  return d;
}

// The element at index k of dist(0 .. n - 1) sorted ascending, without sorting: the smallest v in 0 .. 256 with more than k distances
// <= v.  At most nine counts.
template <class F>
__device__ __forceinline__ int kth_smallest(int n, int k, F dist) {
  int lo = 0, hi = 256;
  while (lo < hi) {
    const int v = (lo + hi) >> 1;
    int cnt = 0;
    for (int j = 0; j < n; j++) cnt += dist(j) <= v;
    if (cnt > k) hi = v; else lo = v + 1;
  }
  return lo;
}

// MapPoint.cc:390: vDists[0.5 * (N - 1)]
__device__ __forceinline__ int median_index(int n) { return (n - 1) >> 1; }

__global__ __launch_bounds__(256) void k_mpd_classify(Args g) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= g.npoints) return;
  const int s = g.start[m], e = g.start[m + 1];
  const int orow = g.out_row ? g.out_row[m] : m;
  const bool ok = s >= 0 && e >= s && e <= g.nobs && e - s <= ORBX_MPDESC_MAX_OBS && orow >= 0 && orow < g.out_rows;
  const int n = e - s;                     // meaningful when ok
  const int c = !ok ? kBad : n == 0 ? kEmpty : n <= g.small_max ? kSmall : n <= g.mid_max ? kMid : kLarge;
  g.cls[m] = c;
  if (c == kBad) { g.best[m] = -2; g.median[m] = -1; }
  else if (c == kEmpty) { g.best[m] = -1; g.median[m] = -1; }
  else if (c == kMid) g.list_mid[atomicAdd(&g.cnt[0], 1)] = m;
  else if (c == kLarge) g.list_large[atomicAdd(&g.cnt[1], 1)] = m;
}

// the chunk's point that owns flat index f: start[p] <= f < start[p + 1] (empty points share their start with the next one)
__device__ __forceinline__ int owner(const int* start, int f) {
  int lo = 0, hi = kChunk;
#pragma unroll
  for (int s = 0; s < 7; s++) {            // 2^7 = kChunk
    const int mid = (lo + hi) >> 1;
    if (start[mid] <= f) lo = mid; else hi = mid;
  }
  return lo;
}
static_assert(kChunk == 128, "owner()'s seven steps");

__global__ __launch_bounds__(kLanes) void k_mpd_small(Args g) {
  __shared__ uint16_t s_row[kSmallCap * kLanes];       // [j][lane]
  __shared__ uint4 s_desc[2 * kStage];
  __shared__ int s_start[kChunk + 1], s_gs[kChunk], s_key[kChunk], s_bad[kChunk], s_wsum[kChunk / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * kChunk;
  // ---- the chunk's small points: a scan of their N
  int inc = 0;
  if (tid < kChunk) {                      // whole waves
    const int m = m0 + tid;
    int n = 0, gs = 0;
    if (m < g.npoints && g.cls[m] == kSmall) { gs = g.start[m]; n = g.start[m + 1] - gs; }   // in range: k_mpd_classify
    s_gs[tid] = gs; s_key[tid] = INT_MAX; s_bad[tid] = 0;
    inc = n;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(inc, o); if (lane >= o) inc += u; }
    if (lane == 63) s_wsum[wave] = inc;
  }
  __syncthreads();
  if (tid < kChunk) {
    int off = 0;
#pragma unroll
    for (int w = 0; w < kChunk / 64; w++) off += w < wave ? s_wsum[w] : 0;
    s_start[tid + 1] = off + inc;
    if (tid == 0) s_start[0] = 0;
  }
  __syncthreads();
  const int total = s_start[kChunk];
  if (total == 0) return;                  // uniform over the workgroup
  // ---- every observation is checked before one addresses the side
  for (int f = tid; f < total; f += kLanes) {
    const int p = owner(s_start, f);
    if (!obs_ok(g, g.obs[s_gs[p] + (f - s_start[p])])) s_bad[p] = 1;
  }
  __syncthreads();
  for (int base = 0; base < total; base += kLanes) {
    // ---- the descriptors of every point this pass touches
    const int lo = s_start[owner(s_start, base)], hi = s_start[owner(s_start, min(base + kLanes, total) - 1) + 1];
    for (int e = lo + tid; e < hi; e += kLanes) {
      const int p = owner(s_start, e);
      if (!s_bad[p]) {
        const uint4* const src = desc_of(g, g.obs[s_gs[p] + (e - s_start[p])]);
        s_desc[2 * (e - lo)] = src[0]; s_desc[2 * (e - lo) + 1] = src[1];
      }
    }
    __syncthreads();
    const int f = base + tid;
    if (f < total) {
      const int p = owner(s_start, f);
      if (!s_bad[p]) {
        const int ps = s_start[p], n = s_start[p + 1] - ps, i = f - ps, off = ps - lo;
        const D8 mine = d8(s_desc[2 * (off + i)], s_desc[2 * (off + i) + 1]);
        for (int j = 0; j < n; j++) s_row[j * kLanes + tid] = (uint16_t)hamming(mine, d8(s_desc[2 * (off + j)], s_desc[2 * (off + j) + 1]));
        const int med = kth_smallest(n, median_index(n), [&](int j) { return (int)s_row[j * kLanes + tid]; });
        atomicMin(&s_key[p], (med << 11) | i);
      }
    }
    __syncthreads();                       // the next pass overwrites s_desc
  }
  // ---- a thread per point: the winner and its 32 bytes
  if (tid < kChunk) {
    const int m = m0 + tid;
    if (m < g.npoints && g.cls[m] == kSmall) {
      if (s_bad[tid]) { g.best[m] = -2; g.median[m] = -1; }
      else {
        const int key = s_key[tid], b = key & 2047;
        g.best[m] = b; g.median[m] = key >> 11;
        const uint4* const src = desc_of(g, g.obs[s_gs[tid] + b]);
        const size_t orow = g.out_row ? g.out_row[m] : m;        // in range: k_mpd_classify
        g.out_desc[2 * orow] = src[0]; g.out_desc[2 * orow + 1] = src[1];
      }
    }
  }
}

template <bool MATRIX>
__global__ __launch_bounds__(MATRIX ? kMidCap : ORBX_MPDESC_MAX_OBS) void k_mpd_point(Args g) {
  constexpr int T = MATRIX ? kMidCap : ORBX_MPDESC_MAX_OBS;
  extern __shared__ __align__(16) uint8_t smem[];
  __shared__ int s_key, s_bad;
  uint4* const s_desc = (uint4*)smem;                              // [T][2]
  uint16_t* const s_row = (uint16_t*)(smem + (size_t)T * 32);      // MATRIX: [j][lane]
  const int tid = threadIdx.x;
  const int32_t* const list = MATRIX ? g.list_mid : g.list_large;
  const int count = g.cnt[MATRIX ? 0 : 1];
  for (int idx = blockIdx.x; idx < count; idx += gridDim.x) {
    const int m = list[idx];
    const int s = g.start[m], n = g.start[m + 1] - s;              // in range, n <= T: k_mpd_classify
    if (tid == 0) { s_key = INT_MAX; s_bad = 0; }
    __syncthreads();
    int2 o = make_int2(0, 0);
    if (tid < n) {
      o = g.obs[s + tid];
      if (!obs_ok(g, o)) s_bad = 1;
    }
    __syncthreads();
    if (s_bad) {                           // uniform over the workgroup
      if (tid == 0) { g.best[m] = -2; g.median[m] = -1; }
    } else {
      if (tid < n) {
        const uint4* const src = desc_of(g, o);
        s_desc[2 * tid] = src[0]; s_desc[2 * tid + 1] = src[1];
      }
      __syncthreads();
      if (tid < n) {
        const D8 mine = d8(s_desc[2 * tid], s_desc[2 * tid + 1]);
        int med;
        if (MATRIX) {
          for (int j = 0; j < n; j++) s_row[j * T + tid] = (uint16_t)hamming(mine, d8(s_desc[2 * j], s_desc[2 * j + 1]));
          med = kth_smallest(n, median_index(n), [&](int j) { return (int)s_row[j * T + tid]; });
        } else {
          med = kth_smallest(n, median_index(n), [&](int j) { return hamming(mine, d8(s_desc[2 * j], s_desc[2 * j + 1])); });
        }
        atomicMin(&s_key, (med << 11) | tid);
      }
      __syncthreads();
      const int b = s_key & 2047;
      if (tid == 0) { g.best[m] = b; g.median[m] = s_key >> 11; }
      if (tid < 2) {
        const size_t orow = g.out_row ? g.out_row[m] : m;          // in range: k_mpd_classify
        g.out_desc[2 * orow + tid] = s_desc[2 * b + tid];
      }
    }
    __syncthreads();                       // s_key, s_bad and s_desc are the next point's
  }
}

}  // namespace

struct orbx_mpdesc : orbx::side::Handle {     // scratch: the classes, the two lists and their counters
  int small_max = kSmallCap, mid_max = kMidCap;   // ORBX_MPDESC_SMALL_MAX, ORBX_MPDESC_MID_MAX at create
};

namespace {

using namespace orbx::side;

// what both forms check before anything is copied or launched
int check_select(orbx_mpdesc* m, const char* who, const orbx_mpdesc_side* side, const void* obs, int nobs, const void* obs_start, int npoints,
                 const void* out_desc, int out_rows, const void* best, const void* median) {
  const std::string w(who);
  if (!side) return fail(m, ORBX_E_INVALID, w + "null side");
  if (side->nframes < 1 || side->capacity < 1) return fail(m, ORBX_E_INVALID, w + "nframes and capacity must be at least 1");
  if (!side->d_desc || !side->d_counts) return fail(m, ORBX_E_INVALID, w + "null buffer in the side");
  if ((long long)side->nframes * (long long)side->capacity > (long long)INT_MAX) return fail(m, ORBX_E_INVALID, w + "nframes * capacity exceeds INT_MAX");
  if (!obs || !obs_start) return fail(m, ORBX_E_INVALID, w + "null obs or obs_start");
  if (!out_desc || !best || !median) return fail(m, ORBX_E_INVALID, w + "null out_desc, best or median");
  if (nobs < 1 || npoints < 1) return fail(m, ORBX_E_INVALID, w + "nobs and npoints must be at least 1");
  if (out_rows < 1) return fail(m, ORBX_E_INVALID, w + "out_rows must be at least 1 (out_rows = " + std::to_string(out_rows) + ")");
  return ORBX_OK;
}

}  // namespace

extern "C" {

int orbx_mpdesc_create(orbx_mpdesc** out, int device) {
  return create_handle(out, device, "orbx_mpdesc_create", orbx_mpdesc_destroy, [](orbx_mpdesc* m) {
    m->small_max = env_int("ORBX_MPDESC_SMALL_MAX", 0, kSmallCap, kSmallCap);
    m->mid_max = env_int("ORBX_MPDESC_MID_MAX", 0, kMidCap, kMidCap);
    const char* e = allow_lds((const void*)k_mpd_point<true>, kMidLds);
    return e ? e : allow_lds((const void*)k_mpd_point<false>, kLargeLds);
  });
}

void orbx_mpdesc_destroy(orbx_mpdesc* m) { destroy_handle(m); }

const char* orbx_mpdesc_last_error(const orbx_mpdesc* m) { return last_error(m); }

int orbx_mpdesc_select_device(orbx_mpdesc* m, const orbx_mpdesc_side* side, const orbx_mpdesc_obs* d_obs, int nobs, const int32_t* d_obs_start,
                              int npoints, const int32_t* d_out_row, uint8_t* d_out_desc, int out_rows, int32_t* d_best, int32_t* d_median,
                              void* stream) {
  if (!m) return ORBX_E_INVALID;
  const char* who = "orbx_mpdesc_select_device: ";
  int rc = check_select(m, who, side, d_obs, nobs, d_obs_start, npoints, d_out_desc, out_rows, d_best, d_median);
  if (rc != ORBX_OK) return rc;
  if (((uintptr_t)side->d_desc | (uintptr_t)d_out_desc) & 15) return fail(m, ORBX_E_INVALID, std::string(who) + "d_desc and d_out_desc must be 16-byte aligned");
  rc = same_device(m, who, {side->d_desc, side->d_counts, d_obs, d_obs_start, d_out_row, d_out_desc, d_best, d_median}, "the handle");
  if (rc != ORBX_OK) return rc;
  ORBX_SIDE_HIP(m, hipSetDevice(m->device));
  Layout lay;
  const size_t o_cnt = lay.add(2 * sizeof(int32_t)), o_cls = lay.add((size_t)npoints * 4), o_mid = lay.add((size_t)npoints * 4);
  const size_t o_large = lay.add((size_t)npoints * 4);
  if ((rc = grow(m, &m->scratch, lay.size)) != ORBX_OK) return rc;
  uint8_t* const d = m->scratch.p;
  Args g;
  g.desc = side->d_desc; g.counts = side->d_counts; g.obs = (const int2*)d_obs; g.start = d_obs_start; g.out_row = d_out_row;
  g.out_desc = (uint4*)d_out_desc; g.best = d_best; g.median = d_median;
  g.cls = (int32_t*)(d + o_cls); g.list_mid = (int32_t*)(d + o_mid); g.list_large = (int32_t*)(d + o_large); g.cnt = (int32_t*)(d + o_cnt);
  g.nframes = side->nframes; g.cap = side->capacity; g.nobs = nobs; g.npoints = npoints; g.out_rows = out_rows;
  g.small_max = m->small_max; g.mid_max = m->mid_max;
  hipStream_t st = stream ? (hipStream_t)stream : m->st;
  if ((rc = wait_previous(m, st)) != ORBX_OK) return rc;
  ORBX_SIDE_HIP(m, hipMemsetAsync(g.cnt, 0, 2 * sizeof(int32_t), st));
  hipLaunchKernelGGL(k_mpd_classify, dim3(((unsigned)npoints + 255) / 256), dim3(256), 0, st, g);
  hipLaunchKernelGGL(k_mpd_small, dim3(((unsigned)npoints + kChunk - 1) / kChunk), dim3(kLanes), 0, st, g);
  hipLaunchKernelGGL(k_mpd_point<true>, dim3((unsigned)std::min(npoints, kMidGrid)), dim3(kMidCap), kMidLds, st, g);
  hipLaunchKernelGGL(k_mpd_point<false>, dim3((unsigned)std::min(npoints, kLargeGrid)), dim3(ORBX_MPDESC_MAX_OBS), kLargeLds, st, g);
  return record_call(m, st);
}

int orbx_mpdesc_select(orbx_mpdesc* m, const orbx_mpdesc_side* side, const orbx_mpdesc_obs* obs, int nobs, const int32_t* obs_start, int npoints,
                       const int32_t* out_row, uint8_t* out_desc, int out_rows, int32_t* best, int32_t* median) {
  if (!m) return ORBX_E_INVALID;
  const char* who = "orbx_mpdesc_select: ";
  int rc = check_select(m, who, side, obs, nobs, obs_start, npoints, out_desc, out_rows, best, median);
  if (rc != ORBX_OK) return rc;
  Stager io;
  const size_t nf = (size_t)side->nframes;
  const size_t o_desc = io.in(side->d_desc, nf * side->capacity * 32), o_counts = io.in(side->d_counts, nf * 8);
  const size_t o_obs = io.in(obs, (size_t)nobs * sizeof(orbx_mpdesc_obs)), o_start = io.in(obs_start, ((size_t)npoints + 1) * 4);
  const size_t o_row = out_row ? io.in(out_row, (size_t)npoints * 4) : 0;
  const size_t o_out = io.out(out_desc, (size_t)out_rows * 32, true), o_best = io.out(best, (size_t)npoints * 4), o_med = io.out(median, (size_t)npoints * 4);
  if ((rc = upload(m, io)) != ORBX_OK) return rc;
  uint8_t* const d = m->io.p;
  const orbx_mpdesc_side ds = {d + o_desc, (const int32_t*)(d + o_counts), side->nframes, side->capacity};
  rc = orbx_mpdesc_select_device(m, &ds, (const orbx_mpdesc_obs*)(d + o_obs), nobs, (const int32_t*)(d + o_start), npoints,
                                 out_row ? (const int32_t*)(d + o_row) : nullptr, d + o_out, out_rows, (int32_t*)(d + o_best), (int32_t*)(d + o_med),
                                 m->st);
  if (rc != ORBX_OK) return rc;
  return download(m, io);
}

}  // extern "C"
