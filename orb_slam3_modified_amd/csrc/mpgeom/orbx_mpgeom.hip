// The batched MapPoint::UpdateNormalAndDepth (include/orbx_mpgeom.h, src/MapPoint.cc:426-494): for M map points at once, the view direction
// and the scale-invariance range, written in place into the table of map points the projection fronts read.  view_term and finish_point are
// the specification, stated once for the host twin and the kernels; so are the checks (classify, names_row).  The work is gathers, three
// divisions and a square root per observation; the ordered sum is three additions per observation and is never reassociated.  Three
// launches whatever the points are, no host synchronisation:
//
// k_mpg_check: a thread per point.  obs_start, N, the table row, the reference observation and its octave are checked before any of them
//   addresses memory; the point's class {malformed, empty, small, large} goes to the handle's memory, malformed and empty points get their
//   d_n here, large points are appended to an index list (an integer atomic counter: the list's order varies, no result depends on it).
// k_mpg_small (N <= small_max <= 64): A LANE PER OBSERVATION.  Most points have 2 - 30 observations, which would leave a wave per point
//   idle.  A wave owns 16 consecutive points: a scan of their N gives every observation a flat index, and the wave walks them in passes of
//   whole points, at most 64 observations a pass, so a point's observations never split across passes or waves.  Every lane checks its
//   observation and computes its own q(d, len) term; then the head lane of each point's segment adds its segment's terms in list order,
//   reading lane + k for k = 0 .. N - 1 (all segments of the pass at once; no scan: a scan reassociates).  The sums wait in LDS until the
//   wave's passes are over; then a lane per point does steps 3 - 5 and writes its row.
// k_mpg_large (N <= 1024): a wave per point of the large list, walked with a grid stride (the list's length is known on the device only).
//   Each trip computes 64 terms into registers; every lane then adds them in order from lane 0 .. 63 (the same sum in all lanes), lane 0
//   writes.
// The row is written as one 16-byte store (normal, max_inv) and two dword stores (min_inv, max_dist); pos and pad are never written.
// The float expressions are compiled with -ffp-contract=off and hipcc's correctly rounded fp32 divide and sqrt; no fast-math flag.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>

#include "../side/orbx_handle.h"
#include "../side/orbx_front_device.h"
#include "../../../include/orbx_mpgeom.h"

namespace {

using orbx::side::front::sum3;

constexpr int kSmallCap = 64;             // the largest N the lane-per-observation form can take: a pass is one wave
constexpr int kSmallDefault = 16;         // the routing boundary: at 20 000 points of 0 .. 40 observations 0, 8 and 16 run in 0.070 - 0.072 ms, 32 in
                                          // 0.080, 64 in 0.088 (profiles/mpgeom_times_r26.txt)
constexpr int kPts = 16;                  // points of one wave of k_mpg_small
constexpr int kWaves = 4;                 // waves of a workgroup of either form
constexpr int kLargeGrid = 512;           // workgroups that walk the large list
static_assert(sizeof(orbx_keypoint) == 28 && sizeof(orbx_mpgeom_obs) == 8 && sizeof(orbx_frustum_point) == 48, "record sizes");
static_assert(ORBX_MPGEOM_MAX_LEVELS == 16 && kSmallCap == 64 && kPts == 16, "the unrolled level pick; a pass is a wave; the scan's four steps");

enum : int32_t { kBad = 0, kEmpty = 1, kSmall = 2, kLarge = 3 };

struct Args {
  const orbx_keypoint* kps; const int32_t* counts; const int32_t* nleft; const float4* centres;
  const int2* obs; const int32_t* start; const int2* ref; const int32_t* row; float* table;
  int32_t* n; float* min_dist;
  int32_t* cls; int32_t* list; int32_t* cnt;      // the handle's: the classes, the large points and their number
  int nframes, cap, nobs, npoints, table_rows, nlevels, small_max;
  float sf[ORBX_MPGEOM_MAX_LEVELS];               // the last factor repeated past nlevels - 1
  float sf_last;
};

// ------------------------------------------------------------------------------------------------------------------- the specification
template <bool kRecip>
__host__ __device__ inline float quot(float a, float b) { return kRecip ? a * (1.0f / b) : a / b; }

// step 2's term for one observation: (P - C) / |P - C|
template <bool kTree, bool kRecip>
__host__ __device__ inline void view_term(const float* P, const float* C, float* t) {
  const float d[3] = {P[0] - C[0], P[1] - C[1], P[2] - C[2]};
  const float len = sqrtf(sum3<kTree>(d[0] * d[0], d[1] * d[1], d[2] * d[2]));
  for (int k = 0; k < 3; k++) t[k] = quot<kRecip>(d[k], len);
}

struct Geom { float normal[3], max_inv, min_inv, max_dist, min_dist; };

// steps 3 .. 5: C the reference keyframe's LEFT centre, sf_level its keypoint's scale factor
template <bool kTree, bool kRecip>
__host__ __device__ inline Geom finish_point(const float* P, const float* C, const float* normal, int n, float sf_level, float sf_last) {
  const float PC[3] = {P[0] - C[0], P[1] - C[1], P[2] - C[2]};
  const float dist = sqrtf(sum3<kTree>(PC[0] * PC[0], PC[1] * PC[1], PC[2] * PC[2]));
  Geom o;
  o.max_dist = dist * sf_level;
  o.min_dist = o.max_dist / sf_last;
  const float fn = (float)n;
  for (int k = 0; k < 3; k++) o.normal[k] = quot<kRecip>(normal[k], fn);
  o.max_inv = 1.2f * o.max_dist;
  o.min_inv = 0.8f * o.min_dist;
  return o;
}

// (frame, row) names a row the side holds, on a frame whose nleft is sound
__host__ __device__ inline bool names_row(const Args& g, int2 o) {
  if (o.x < 0 || o.x >= g.nframes || o.y < 0) return false;
  const int count = g.counts[2 * o.x], rows = count < g.cap ? count : g.cap;
  if (o.y >= rows) return false;
  if (g.nleft) {
    const int nl = g.nleft[o.x];
    if (nl < -1 || nl > rows) return false;
  }
  return true;
}
// its camera's centre as an index into centres (the device reads 16 bytes there, the host twin three floats); names_row(o) holds
__host__ __device__ inline int centre_of(const Args& g, int2 o) {
  int right = 0;
  if (g.nleft) {
    const int nl = g.nleft[o.x];
    right = nl >= 0 && o.y >= nl;
  }
  return 2 * o.x + right;
}
__host__ __device__ inline int octave_of(const Args& g, int2 o) { return g.kps[(size_t)o.x * g.cap + o.y].octave; }

// scale_factors[level] with constant indices only: sf is a kernel argument
__host__ __device__ inline float pick_sf(const float* sf, int level) {
  float s = sf[0];
#pragma unroll
  for (int n = 1; n < ORBX_MPGEOM_MAX_LEVELS; n++)
    if (level == n) s = sf[n];
  return s;
}

// What is checked of a point before its observations are walked.  Every point: obs_start, N, the table row.  N > 0: the reference
// observation and its octave.
__host__ __device__ inline int classify(const Args& g, int m) {
  const int s = g.start[m], e = g.start[m + 1];
  const int r = g.row ? g.row[m] : m;
  if (!(s >= 0 && e >= s && e <= g.nobs && e - s <= ORBX_MPGEOM_MAX_OBS && r >= 0 && r < g.table_rows)) return kBad;
  if (e == s) return kEmpty;
  const int2 ref = g.ref[m];
  if (!names_row(g, ref)) return kBad;
  const int level = octave_of(g, ref);
  if (level < 0 || level >= g.nlevels) return kBad;
  return e - s <= g.small_max ? kSmall : kLarge;
}

// ---------------------------------------------------------------------------------------------------------------------------- the kernels
typedef float Float4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void k_mpg_check(Args g) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= g.npoints) return;
  const int c = classify(g, m);
  g.cls[m] = c;
  if (c == kBad) g.n[m] = -2;
  else if (c == kEmpty) g.n[m] = 0;
  else if (c == kLarge) g.list[atomicAdd(&g.cnt[0], 1)] = m;
}

// steps 3 .. 5 and the stores for point m of n sound observations; classify(m) was small or large
template <bool kTree, bool kRecip>
__device__ __forceinline__ void write_point(const Args& g, int m, int n, const float* normal) {
  const size_t r = g.row ? g.row[m] : m;
  const float4 P = ((const float4*)g.table)[3 * r];
  const int2 ref = g.ref[m];
  const float4 C = g.centres[2 * ref.x];
  const float p[3] = {P.x, P.y, P.z}, c[3] = {C.x, C.y, C.z};
  const Geom o = finish_point<kTree, kRecip>(p, c, normal, n, pick_sf(g.sf, octave_of(g, ref)), g.sf_last);
  ((Float4*)g.table)[3 * r + 1] = Float4{o.normal[0], o.normal[1], o.normal[2], o.max_inv};
  g.table[12 * r + 3] = o.min_inv;
  g.table[12 * r + 8] = o.max_dist;
  g.n[m] = n;
  if (g.min_dist) g.min_dist[m] = o.min_dist;
}

// a lane's term: observation i of point m.  false: the observation is malformed
template <bool kTree, bool kRecip>
__device__ __forceinline__ bool lane_term(const Args& g, int m, int i, float* t) {
  const int2 o = g.obs[g.start[m] + i];         // in range: k_mpg_check
  if (!names_row(g, o)) return false;
  const size_t r = g.row ? g.row[m] : m;
  const float4 P = ((const float4*)g.table)[3 * r];
  const float4 C = g.centres[centre_of(g, o)];
  const float p[3] = {P.x, P.y, P.z}, c[3] = {C.x, C.y, C.z};
  view_term<kTree, kRecip>(p, c, t);
  return true;
}

template <bool kTree, bool kRecip>
__global__ __launch_bounds__(64 * kWaves) void k_mpg_small(Args g) {
  __shared__ int s_start[kWaves][kPts + 1];
  __shared__ float s_acc[kWaves][kPts][3];
  __shared__ int s_bad[kWaves][kPts];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m0 = (blockIdx.x * kWaves + wave) * kPts;
  int* const st = s_start[wave];
  // ---- a lane per point: a scan of the small points' N
  const int mine = m0 + lane;
  int n = 0;
  if (lane < kPts && mine < g.npoints && g.cls[mine] == kSmall) n = g.start[mine + 1] - g.start[mine];   // 1 .. small_max: k_mpg_check
  int inc = n;
#pragma unroll
  for (int o = 1; o < kPts; o <<= 1) { const int u = __shfl_up(inc, o); if (lane >= o) inc += u; }
  if (lane < kPts) st[lane + 1] = inc;
  if (lane == 0) st[0] = 0;
  __syncthreads();
  // ---- passes of whole points, at most 64 observations each
  int p0 = 0;
  while (p0 < kPts) {                                    // wave-uniform
    const int base = __builtin_amdgcn_readfirstlane(st[p0]);
    int p1 = p0 + 1;
    while (p1 < kPts && __builtin_amdgcn_readfirstlane(st[p1 + 1]) - base <= 64) p1++;
    const int count = __builtin_amdgcn_readfirstlane(st[p1]) - base;   // <= 64: one point's N at least, and a point has at most 64
    if (count > 0) {
      const int f = base + lane;
      const bool live = lane < count;
      int p = 0;                                          // the last point with st[p] <= f: empty points share their start with the next
      if (live) {
        int hi = kPts;
#pragma unroll
        for (int s = 0; s < 4; s++) { const int mid = (p + hi) >> 1; if (st[mid] <= f) p = mid; else hi = mid; }
      }
      const int i = f - st[p], np = st[p + 1] - st[p];
      float t[3] = {0.0f, 0.0f, 0.0f};
      bool bad = false;
      if (live) bad = !lane_term<kTree, kRecip>(g, m0 + p, i, t);
      const unsigned long long badmask = __ballot(bad);
      // ---- the head lane of each segment adds its terms in list order
      const bool head = live && i == 0;
      float acc[3] = {0.0f, 0.0f, 0.0f};
      for (int k = 0; __any(head && k < np); k++) {      // wave-uniform
        const float v0 = __shfl(t[0], lane + k), v1 = __shfl(t[1], lane + k), v2 = __shfl(t[2], lane + k);
        if (head && k < np) { acc[0] = acc[0] + v0; acc[1] = acc[1] + v1; acc[2] = acc[2] + v2; }
      }
      if (head) {
        const unsigned long long seg = np >= 64 ? ~0ull : ((1ull << np) - 1ull);
        s_bad[wave][p] = ((badmask >> lane) & seg) != 0ull;
        s_acc[wave][p][0] = acc[0]; s_acc[wave][p][1] = acc[1]; s_acc[wave][p][2] = acc[2];
      }
    }
    p0 = p1;
  }
  __syncthreads();                                       // every wave arrives once, its passes over
  // ---- a lane per point: steps 3 - 5
  if (n > 0) {
    if (s_bad[wave][lane]) g.n[mine] = -2;
    else {
      const float normal[3] = {s_acc[wave][lane][0], s_acc[wave][lane][1], s_acc[wave][lane][2]};
      write_point<kTree, kRecip>(g, mine, n, normal);
    }
  }
}

template <bool kTree, bool kRecip>
__global__ __launch_bounds__(64 * kWaves) void k_mpg_large(Args g) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int count = g.cnt[0];
  for (int idx = blockIdx.x * kWaves + wave; idx < count; idx += gridDim.x * kWaves) {   // wave-uniform
    const int m = g.list[idx];
    const int n = g.start[m + 1] - g.start[m];           // small_max < n <= 1024: k_mpg_check
    float acc[3] = {0.0f, 0.0f, 0.0f};
    bool bad = false;
    for (int base = 0; base < n && !bad; base += 64) {
      float t[3] = {0.0f, 0.0f, 0.0f};
      bool mybad = false;
      if (base + lane < n) mybad = !lane_term<kTree, kRecip>(g, m, base + lane, t);
      bad = __any(mybad);
      const int c = min(64, n - base);
      for (int k = 0; k < c; k++) {                      // every lane holds the same ordered sum
        acc[0] = acc[0] + __shfl(t[0], k); acc[1] = acc[1] + __shfl(t[1], k); acc[2] = acc[2] + __shfl(t[2], k);
      }
    }
    if (lane == 0) {
      if (bad) g.n[m] = -2;
      else write_point<kTree, kRecip>(g, m, n, acc);
    }
  }
}
}  // namespace

struct orbx_mpgeom : orbx::side::Handle {     // scratch: the classes, the large list and its counter
  int small_max = kSmallDefault;              // ORBX_MPGEOM_SMALL_MAX at create
};

namespace {

using namespace orbx::side;

// what every form checks before anything is computed, copied or launched; the reason, or nullptr
const char* call_problem(const orbx_mpgeom_side* side, const void* obs, int nobs, const void* obs_start, int npoints, const void* ref, const void* table,
                         int table_rows, const float* scale_factors, int nlevels, int sum_order, int div_kind, const void* n) {
  if (!side) return "null side";
  if (!side->d_kps || !side->d_counts || !side->d_centres) return "null buffer in the side";
  if (!obs || !obs_start || !ref) return "null obs, obs_start or ref";
  if (!table || !scale_factors || !n) return "null table, scale_factors or n";
  if (side->nframes < 1 || side->capacity < 1) return "nframes and capacity must be at least 1";
  if ((long long)side->nframes * (long long)side->capacity > (long long)INT_MAX) return "nframes * capacity exceeds INT_MAX";
  if (nobs < 1 || npoints < 1 || table_rows < 1) return "nobs, npoints and table_rows must be at least 1";
  if (nlevels < 1 || nlevels > ORBX_MPGEOM_MAX_LEVELS) return "nlevels must be in 1 .. 16";
  if (sum_order != ORBX_FRUSTUM_SUM_LTR && sum_order != ORBX_FRUSTUM_SUM_TREE) return "unknown sum_order";
  if (div_kind != ORBX_MPGEOM_DIV_QUOTIENT && div_kind != ORBX_MPGEOM_DIV_RECIPROCAL) return "unknown div_kind";
  return nullptr;
}

void fill_args(Args* g, const orbx_mpgeom_side* side, const orbx_mpgeom_obs* obs, int nobs, const int32_t* obs_start, int npoints,
               const orbx_mpgeom_obs* ref, const int32_t* row, orbx_frustum_point* table, int table_rows, const float* scale_factors, int nlevels,
               int32_t* n, float* min_dist) {
  g->kps = side->d_kps; g->counts = side->d_counts; g->nleft = side->d_nleft; g->centres = (const float4*)side->d_centres;
  g->obs = (const int2*)obs; g->start = obs_start; g->ref = (const int2*)ref; g->row = row; g->table = (float*)table;
  g->n = n; g->min_dist = min_dist;
  g->cls = nullptr; g->list = nullptr; g->cnt = nullptr;
  g->nframes = side->nframes; g->cap = side->capacity; g->nobs = nobs; g->npoints = npoints; g->table_rows = table_rows; g->nlevels = nlevels;
  g->small_max = kSmallDefault;
  for (int l = 0; l < ORBX_MPGEOM_MAX_LEVELS; l++) g->sf[l] = scale_factors[l < nlevels ? l : nlevels - 1];
  g->sf_last = scale_factors[nlevels - 1];
}

// the host twin's loop
template <bool kTree, bool kRecip>
void reference_loop(const Args& g) {
  for (int m = 0; m < g.npoints; m++) {
    const int c = classify(g, m);
    if (c == kBad) { g.n[m] = -2; continue; }
    if (c == kEmpty) { g.n[m] = 0; continue; }
    const int s = g.start[m], n = g.start[m + 1] - s;
    bool bad = false;
    for (int i = 0; i < n && !bad; i++) bad = !names_row(g, g.obs[s + i]);
    if (bad) { g.n[m] = -2; continue; }
    float* const rec = g.table + 12 * (size_t)(g.row ? g.row[m] : m);
    float normal[3] = {0.0f, 0.0f, 0.0f};
    for (int i = 0; i < n; i++) {
      float t[3];
      view_term<kTree, kRecip>(rec, (const float*)g.centres + 4 * centre_of(g, g.obs[s + i]), t);
      for (int k = 0; k < 3; k++) normal[k] = normal[k] + t[k];
    }
    const int2 ref = g.ref[m];
    const Geom o = finish_point<kTree, kRecip>(rec, (const float*)g.centres + 8 * ref.x, normal, n, g.sf[octave_of(g, ref)], g.sf_last);
    rec[3] = o.min_inv;
    rec[4] = o.normal[0]; rec[5] = o.normal[1]; rec[6] = o.normal[2]; rec[7] = o.max_inv;
    rec[8] = o.max_dist;
    g.n[m] = n;
    if (g.min_dist) g.min_dist[m] = o.min_dist;
  }
}

}  // namespace

extern "C" {

int orbx_mpgeom_create(orbx_mpgeom** out, int device) {
  return create_handle(out, device, "orbx_mpgeom_create", orbx_mpgeom_destroy, [](orbx_mpgeom* g) -> const char* {
    g->small_max = env_int("ORBX_MPGEOM_SMALL_MAX", 0, kSmallCap, kSmallDefault);
    return nullptr;
  });
}

void orbx_mpgeom_destroy(orbx_mpgeom* g) { destroy_handle(g); }

const char* orbx_mpgeom_last_error(const orbx_mpgeom* g) { return last_error(g); }

int orbx_mpgeom_update_device(orbx_mpgeom* h, const orbx_mpgeom_side* side, const orbx_mpgeom_obs* d_obs, int nobs, const int32_t* d_obs_start,
                              int npoints, const orbx_mpgeom_obs* d_ref, const int32_t* d_row, orbx_frustum_point* d_table, int table_rows,
                              const float* scale_factors, int nlevels, int sum_order, int div_kind, int32_t* d_n, float* d_min_dist, void* stream) {
  if (!h) return ORBX_E_INVALID;
  const std::string who = "orbx_mpgeom_update_device: ";
  if (const char* e = call_problem(side, d_obs, nobs, d_obs_start, npoints, d_ref, d_table, table_rows, scale_factors, nlevels, sum_order, div_kind, d_n))
    return fail(h, ORBX_E_INVALID, who + e);
  if (((uintptr_t)d_table | (uintptr_t)side->d_centres) & 15) return fail(h, ORBX_E_INVALID, who + "d_table and d_centres must be 16-byte aligned");
  int rc = same_device(h, who.c_str(), {side->d_kps, side->d_counts, side->d_nleft, side->d_centres, d_obs, d_obs_start, d_ref, d_row, d_table, d_n,
                                        d_min_dist}, "the handle");
  if (rc != ORBX_OK) return rc;
  ORBX_SIDE_HIP(h, hipSetDevice(h->device));
  Layout lay;
  const size_t o_cnt = lay.add(sizeof(int32_t)), o_cls = lay.add((size_t)npoints * 4), o_list = lay.add((size_t)npoints * 4);
  if ((rc = grow(h, &h->scratch, lay.size)) != ORBX_OK) return rc;
  uint8_t* const d = h->scratch.p;
  Args g;
  fill_args(&g, side, d_obs, nobs, d_obs_start, npoints, d_ref, d_row, d_table, table_rows, scale_factors, nlevels, d_n, d_min_dist);
  g.cls = (int32_t*)(d + o_cls); g.list = (int32_t*)(d + o_list); g.cnt = (int32_t*)(d + o_cnt);
  g.small_max = h->small_max;
  hipStream_t st = stream ? (hipStream_t)stream : h->st;
  if ((rc = wait_previous(h, st)) != ORBX_OK) return rc;
  ORBX_SIDE_HIP(h, hipMemsetAsync(g.cnt, 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(k_mpg_check, dim3(((unsigned)npoints + 255) / 256), dim3(256), 0, st, g);
  const dim3 small(((unsigned)npoints + kWaves * kPts - 1) / (kWaves * kPts)), large((unsigned)std::min((npoints + kWaves - 1) / kWaves, kLargeGrid));
  const dim3 block(64 * kWaves);
  const bool tree = sum_order == ORBX_FRUSTUM_SUM_TREE, recip = div_kind == ORBX_MPGEOM_DIV_RECIPROCAL;
#define ORBX_MPGEOM_LAUNCH(T, R)                                                   \
  do {                                                                             \
    hipLaunchKernelGGL((k_mpg_small<T, R>), small, block, 0, st, g);               \
    hipLaunchKernelGGL((k_mpg_large<T, R>), large, block, 0, st, g);               \
  } while (0)
  if (tree && recip) ORBX_MPGEOM_LAUNCH(true, true);
  else if (tree) ORBX_MPGEOM_LAUNCH(true, false);
  else if (recip) ORBX_MPGEOM_LAUNCH(false, true);
  else ORBX_MPGEOM_LAUNCH(false, false);
#undef ORBX_MPGEOM_LAUNCH
  return record_call(h, st);
}

int orbx_mpgeom_update(orbx_mpgeom* h, const orbx_mpgeom_side* side, const orbx_mpgeom_obs* obs, int nobs, const int32_t* obs_start, int npoints,
                       const orbx_mpgeom_obs* ref, const int32_t* row, orbx_frustum_point* table, int table_rows, const float* scale_factors,
                       int nlevels, int sum_order, int div_kind, int32_t* n, float* min_dist) {
  if (!h) return ORBX_E_INVALID;
  const std::string who = "orbx_mpgeom_update: ";
  if (const char* e = call_problem(side, obs, nobs, obs_start, npoints, ref, table, table_rows, scale_factors, nlevels, sum_order, div_kind, n))
    return fail(h, ORBX_E_INVALID, who + e);
  Stager io;
  const size_t nf = (size_t)side->nframes;
  const size_t o_kps = io.in(side->d_kps, nf * side->capacity * sizeof(orbx_keypoint)), o_counts = io.in(side->d_counts, nf * 8);
  const size_t o_nleft = side->d_nleft ? io.in(side->d_nleft, nf * 4) : 0, o_centres = io.in(side->d_centres, nf * 32);
  const size_t o_obs = io.in(obs, (size_t)nobs * sizeof(orbx_mpgeom_obs)), o_start = io.in(obs_start, ((size_t)npoints + 1) * 4);
  const size_t o_ref = io.in(ref, (size_t)npoints * sizeof(orbx_mpgeom_obs)), o_row = row ? io.in(row, (size_t)npoints * 4) : 0;
  const size_t o_table = io.out(table, (size_t)table_rows * sizeof(orbx_frustum_point), true), o_n = io.out(n, (size_t)npoints * 4);
  const size_t o_min = io.out(min_dist, (size_t)npoints * 4, true);
  int rc = upload(h, io);
  if (rc != ORBX_OK) return rc;
  uint8_t* const d = h->io.p;
  const orbx_mpgeom_side ds = {(const orbx_keypoint*)(d + o_kps), (const int32_t*)(d + o_counts), side->d_nleft ? (const int32_t*)(d + o_nleft) : nullptr,
                               (const float*)(d + o_centres), side->nframes, side->capacity};
  rc = orbx_mpgeom_update_device(h, &ds, (const orbx_mpgeom_obs*)(d + o_obs), nobs, (const int32_t*)(d + o_start), npoints,
                                 (const orbx_mpgeom_obs*)(d + o_ref), row ? (const int32_t*)(d + o_row) : nullptr, (orbx_frustum_point*)(d + o_table),
                                 table_rows, scale_factors, nlevels, sum_order, div_kind, (int32_t*)(d + o_n), min_dist ? (float*)(d + o_min) : nullptr,
                                 h->st);
  if (rc != ORBX_OK) return rc;
  return download(h, io);
}

int orbx_mpgeom_update_reference(const orbx_mpgeom_side* side, const orbx_mpgeom_obs* obs, int nobs, const int32_t* obs_start, int npoints,
                                 const orbx_mpgeom_obs* ref, const int32_t* row, orbx_frustum_point* table, int table_rows, const float* scale_factors,
                                 int nlevels, int sum_order, int div_kind, int32_t* n, float* min_dist) {
  if (const char* e = call_problem(side, obs, nobs, obs_start, npoints, ref, table, table_rows, scale_factors, nlevels, sum_order, div_kind, n))
    return create_fail(ORBX_E_INVALID, "orbx_mpgeom_update_reference", e);
  Args g;
  fill_args(&g, side, obs, nobs, obs_start, npoints, ref, row, table, table_rows, scale_factors, nlevels, n, min_dist);
  const bool tree = sum_order == ORBX_FRUSTUM_SUM_TREE, recip = div_kind == ORBX_MPGEOM_DIV_RECIPROCAL;
  if (tree && recip) reference_loop<true, true>(g);
  else if (tree) reference_loop<true, false>(g);
  else if (recip) reference_loop<false, true>(g);
  else reference_loop<false, false>(g);
  return ORBX_OK;
}

}  // extern "C"
