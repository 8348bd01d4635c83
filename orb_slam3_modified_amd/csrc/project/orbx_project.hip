// The Sophus Tcw * x projection fronts of SearchByProjection(Frame, LastFrame), the relocalization SearchByProjection and Fuse
// (include/orbx_project.h): B (pose, point list) items over the table of map points liborbx_frustum.so reads, written as the rows the three
// batched matchers read.
//
// emit_one<kEmit, kQuat, kTree> is the specification, stated once for the host and the device; what differs is where the level comes from:
// the host twins call libm's log (HostLevel), the kernel counts the caller's thresholds (DeviceLevel).
//
// k_project_check            one workgroup per item: nslots and every index of the row's first nslots against npoints, before any of them
//                            addresses the table; d_nvalid[b] = -1 (malformed) or 0.
// k_project<kEmit, ...>      a lane per (item, slot), 256 slots a workgroup, the workgroups of one item consecutive: the item is
//                            workgroup-uniform, so its constants come through scalar loads from d_items[b], the thresholds and the scale
//                            factors from the kernel arguments.  A lane reads its slot (16 bytes, or one index), gathers what its emitter
//                            needs of the 48-byte record in 16-byte loads and writes its 32-byte row as two 16-byte stores.  nvalid: a ballot
//                            and a popcount per wave, one integer atomic add per wave that counted anything.
// The float expressions are compiled with -ffp-contract=off and hipcc's correctly rounded fp32 divide and sqrt; no fast-math flag.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>

#include "../side/orbx_handle.h"
#include "../../../include/orbx_project.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxLevels = ORBX_FRUSTUM_MAX_LEVELS;
constexpr int kMaxT = kMaxLevels - 1;
enum { kLast = 0, kReloc = 1, kFuse = 2 };
static_assert(sizeof(orbx_frustum_point) == 48 && sizeof(orbx_project_item) == 128 && sizeof(orbx_project_slot) == 16, "record sizes");
static_assert(sizeof(orbx_lastmatch_point) == 32 && sizeof(orbx_projmatch_point) == 32 && sizeof(orbx_fuse_query) == 32, "row sizes");

struct Row { uint32_t w[8]; };   // a row of any of the three consumers, as its 32-bit words
__host__ __device__ inline uint32_t fw(float f) { return __builtin_bit_cast(uint32_t, f); }
__host__ __device__ inline uint32_t iw(int32_t i) { return (uint32_t)i; }

// the skipped row: zero bytes; a fuse query with point = -1
template <int kEmit>
__host__ __device__ inline Row skipped_row() { return {{0u, 0u, 0u, 0u, 0u, 0u, kEmit == kFuse ? 0xFFFFFFFFu : 0u, 0u}}; }

template <bool kTree>
__host__ __device__ inline float sum3(float a, float b, float c) { return kTree ? a + (b + c) : (a + b) + c; }

// Eigen's cross: (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0)
__host__ __device__ inline void cross3(const float* a, const float* b, float* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// Pc = Tcw * P
template <bool kQuat, bool kTree>
__host__ __device__ inline void transform(const orbx_project_item& c, const float* P, float* Pc) {
  if (kQuat) {
    float uv[3], x[3];
    cross3(c.q, P, uv);
    for (int k = 0; k < 3; k++) uv[k] = uv[k] + uv[k];
    cross3(c.q, uv, x);
    for (int k = 0; k < 3; k++) Pc[k] = ((P[k] + c.q[3] * uv[k]) + x[k]) + c.tcw[k];
  } else {
    for (int k = 0; k < 3; k++) Pc[k] = sum3<kTree>(c.Rcw[3 * k] * P[0], c.Rcw[3 * k + 1] * P[1], c.Rcw[3 * k + 2] * P[2]) + c.tcw[k];
  }
}

// One slot below nslots with point < npoints (the caller's): the emitter's gates and its row.  Returns whether the row is valid.
template <int kEmit, bool kQuat, bool kTree, class Points, class Level>
__host__ __device__ inline bool emit_one(const orbx_project_item& c, const Points& points, const int32_t* obs_table, int point, int octave,
                                         float angle, const Level& level, Row* r) {
  *r = skipped_row<kEmit>();
  if (point < 0) return false;
  const orbx_frustum_point p = points(point);
  float Pc[3];
  transform<kQuat, kTree>(c, p.pos, Pc);
  float invz = 0.0f;
  if (kEmit == kLast) {
    invz = 1.0f / Pc[2];
    if (invz < 0.0f) return false;
  }
  if (kEmit == kFuse) {
    if (Pc[2] < 0.0f) return false;
    invz = 1.0f / Pc[2];
  }
  const float u = (c.fx * Pc[0]) / Pc[2] + c.cx, v = (c.fy * Pc[1]) / Pc[2] + c.cy;
  if (kEmit == kFuse) {   // KeyFrame::IsInImage: half-open, a NaN fails
    if (!(u >= c.bounds[0] && u < c.bounds[2])) return false;
    if (!(v >= c.bounds[1] && v < c.bounds[3])) return false;
  } else {                // inclusive edges, a NaN passes
    if (u < c.bounds[0] || u > c.bounds[2]) return false;
    if (v < c.bounds[1] || v > c.bounds[3]) return false;
  }
  if (kEmit == kLast) {
    *r = {{fw(u), fw(v), fw(invz), fw(angle), iw(octave), iw(obs_table[point]), iw(point), 1u}};
    return true;
  }
  float ur = 0.0f;
  if (kEmit == kFuse) {
    const float prod = c.mbf * invz;
    ur = u - prod;
  }
  const float PO[3] = {p.pos[0] - c.Ow[0], p.pos[1] - c.Ow[1], p.pos[2] - c.Ow[2]};
  const float dist = sqrtf(sum3<kTree>(PO[0] * PO[0], PO[1] * PO[1], PO[2] * PO[2]));
  if (dist < p.min_inv || dist > p.max_inv) return false;
  if (kEmit == kFuse) {
    const float dot = sum3<kTree>(PO[0] * p.normal[0], PO[1] * p.normal[1], PO[2] * p.normal[2]);
    if ((double)dot < 0.5 * (double)dist) return false;
  }
  const float ratio = p.max_dist / dist;
  int lvl;
  float scale;
  level(ratio, &lvl, &scale);
  if (kEmit == kReloc) {
    *r = {{fw(u), fw(v), fw(angle), iw(lvl), iw(point), 1u, 0u, 0u}};
  } else {
    const float radius = c.th * scale;
    *r = {{fw(u), fw(v), fw(radius), fw(ur), iw(lvl - 1), iw(lvl), iw(point), 0u}};
  }
  return true;
}

// ---------------------------------------------------------------------------------------------------------------- the level on the host
// int nScale = ceil(log(ratio) / mfLogScaleFactor) under each overload of log, then the clamp; outside the range of int (NaN included)
// x86's conversion gives INT_MIN, which the clamp raises to 0 (include/orbx_frustum.h, step 9 and Limits)
struct HostLevel {
  float lsf; int nlevels, log_kind; const float* sf;
  void operator()(float ratio, int* lvl, float* scale) const {
    double q;
    if (log_kind == ORBX_FRUSTUM_LOG_FLOAT) {
      const float f = std::log(ratio) / lsf;                    // std::log(float): libm's logf, a float division
      q = std::ceil((double)f);
    } else {
      q = std::ceil(::log((double)ratio) / (double)lsf);        // ::log(double), the float divisor promoted
    }
    int n = 0;
    if (q >= -2147483648.0 && q < 2147483648.0) {
      n = (int)q;
      n = n < 0 ? 0 : n >= nlevels ? nlevels - 1 : n;
    }
    *lvl = n;
    *scale = sf ? sf[n] : 0.0f;
  }
};

struct HostPoints {
  const orbx_frustum_point* t;
  const orbx_frustum_point& operator()(int idx) const { return t[idx]; }
};

const char* options_problem(int rot_kind, int sum_order) {
  if (rot_kind != ORBX_PROJECT_ROT_MATRIX && rot_kind != ORBX_PROJECT_ROT_QUAT) return "unknown rot_kind";
  if (sum_order != ORBX_FRUSTUM_SUM_LTR && sum_order != ORBX_FRUSTUM_SUM_TREE) return "unknown sum_order";
  return nullptr;
}
const char* levels_problem(int nlevels) { return nlevels < 1 || nlevels > kMaxLevels ? "nlevels must be in 1 .. 16" : nullptr; }
const char* thresholds_problem(const float* T, int nlevels) {
  if (const char* e = levels_problem(nlevels)) return e;
  if (!T && nlevels > 1) return "null thresholds";
  for (int n = 0; n + 1 < nlevels; n++) {
    if (!std::isfinite(T[n]) || !(T[n] > 0.0f)) return "thresholds must be finite and positive";
    if (n > 0 && !(T[n] > T[n - 1])) return "thresholds must be strictly increasing";
  }
  return nullptr;
}
const char* log_problem(float lsf, int nlevels, int log_kind) {
  if (const char* e = levels_problem(nlevels)) return e;
  if (log_kind != ORBX_FRUSTUM_LOG_DOUBLE && log_kind != ORBX_FRUSTUM_LOG_FLOAT) return "unknown log_kind";
  if (!(std::isfinite(lsf) && lsf > 0.0f)) return "log_scale_factor must be finite and positive";
  return nullptr;
}

// ---------------------------------------------------------------------------------------------------------------------------- the kernels
struct Args {
  const float4* points; const int32_t* obs; const orbx_project_item* items;
  const void* slots;     // orbx_project_slot rows, or int32 rows (fuse)
  const int32_t* nslots;
  float4* out; int32_t* nvalid;
  int npoints, nitems, mcap, chunks;
  int stride;            // the 32-bit words of one slot: 4 or 1; the point's index is the first
  float T[kMaxT];        // +inf beyond nlevels - 2
  float sf[kMaxLevels];  // fuse: the scale factors, the last repeated beyond nlevels - 1
};

// the number of thresholds below ratio; they ascend strictly, so those are T[0 .. level), and the level's scale factor is picked on the way
struct DeviceLevel {
  const float* T; const float* sf;
  __device__ void operator()(float ratio, int* lvl, float* scale) const {
    int l = 0;
    float s = sf[0];
    if (ratio > 0.0f && ratio != INFINITY) {
#pragma unroll
      for (int n = 0; n < kMaxT; n++)
        if (ratio > T[n]) { l = n + 1; s = sf[n + 1]; }
    }
    *lvl = l;
    *scale = s;
  }
};
struct DevicePoints {
  const float4* t;
  __device__ orbx_frustum_point operator()(int idx) const {
    const float4 a = t[3 * (size_t)idx], b = t[3 * (size_t)idx + 1];
    const float max_dist = ((const float*)(t + 3 * (size_t)idx + 2))[0];
    return {{a.x, a.y, a.z}, a.w, {b.x, b.y, b.z}, b.w, max_dist, {0.0f, 0.0f, 0.0f}};
  }
};

__global__ __launch_bounds__(kThreads) void k_project_check(Args g) {
  const int b = blockIdx.x;
  const int n = g.nslots[b];
  int bad = n < 0 || n > g.mcap;
  if (!bad) {
    const int32_t* row = (const int32_t*)g.slots + (size_t)b * g.mcap * g.stride;
    for (int j = threadIdx.x; j < n; j += kThreads) bad |= row[(size_t)j * g.stride] >= g.npoints;
  }
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) g.nvalid[b] = bad ? -1 : 0;
}

template <int kEmit, bool kQuat, bool kTree>
__global__ __launch_bounds__(kThreads) void k_project(Args g) {
  const int b = (int)(blockIdx.x / (unsigned)g.chunks);
  const int j = (int)(blockIdx.x - (unsigned)b * (unsigned)g.chunks) * kThreads + (int)threadIdx.x;
  // -1 stays -1: a malformed item adds nothing; a sound one only grows from 0
  const bool bad = __hip_atomic_load(g.nvalid + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0;
  const int n = bad ? 0 : g.nslots[b];
  bool valid = false;
  if (j < g.mcap) {
    const size_t slot = (size_t)b * g.mcap + j;
    Row r = skipped_row<kEmit>();
    if (j < n) {
      int point, octave = 0;
      float angle = 0.0f;
      if (kEmit == kFuse) {
        point = ((const int32_t*)g.slots)[slot];
      } else {
        const int4 s = ((const int4*)g.slots)[slot];
        point = s.x; octave = s.y; angle = __int_as_float(s.z);
      }
      valid = emit_one<kEmit, kQuat, kTree>(g.items[b], DevicePoints{g.points}, g.obs, point, octave, angle, DeviceLevel{g.T, g.sf}, &r);
    }
    g.out[2 * slot] = make_float4(__uint_as_float(r.w[0]), __uint_as_float(r.w[1]), __uint_as_float(r.w[2]), __uint_as_float(r.w[3]));
    g.out[2 * slot + 1] = make_float4(__uint_as_float(r.w[4]), __uint_as_float(r.w[5]), __uint_as_float(r.w[6]), __uint_as_float(r.w[7]));
  }
  const int count = __popcll(__ballot(valid));
  if (count > 0 && (threadIdx.x & 63) == 0) atomicAdd(g.nvalid + b, count);
}

template <int kEmit>
void launch(const Args& g, int rot_kind, int sum_order, hipStream_t st) {
  const dim3 grid((unsigned)(g.nitems * g.chunks)), block(kThreads);
  const bool quat = rot_kind == ORBX_PROJECT_ROT_QUAT, tree = sum_order == ORBX_FRUSTUM_SUM_TREE;
  if (quat && tree) hipLaunchKernelGGL((k_project<kEmit, true, true>), grid, block, 0, st, g);
  else if (quat) hipLaunchKernelGGL((k_project<kEmit, true, false>), grid, block, 0, st, g);
  else if (tree) hipLaunchKernelGGL((k_project<kEmit, false, true>), grid, block, 0, st, g);
  else hipLaunchKernelGGL((k_project<kEmit, false, false>), grid, block, 0, st, g);
}

// the host twin of one emitter: the check and the per-slot loop
template <int kEmit>
void reference(const orbx_frustum_point* points, const int32_t* obs, int npoints, const orbx_project_item* items, int nitems, const void* slots,
               const int32_t* nslots, int mcap, const HostLevel& level, int rot_kind, int sum_order, void* out, int32_t* nvalid) {
  const int stride = kEmit == kFuse ? 1 : 4;
  const HostPoints table = {points};
  const bool quat = rot_kind == ORBX_PROJECT_ROT_QUAT, tree = sum_order == ORBX_FRUSTUM_SUM_TREE;
  for (int b = 0; b < nitems; b++) {
    const int32_t* row = (const int32_t*)slots + (size_t)b * mcap * stride;
    bool bad = nslots[b] < 0 || nslots[b] > mcap;
    for (int j = 0; !bad && j < nslots[b]; j++) bad = row[(size_t)j * stride] >= npoints;
    const int n = bad ? 0 : nslots[b];
    int count = 0;
    for (int j = 0; j < mcap; j++) {
      Row r = skipped_row<kEmit>();
      if (j < n) {
        const int32_t* s = row + (size_t)j * stride;
        const int point = s[0], octave = kEmit == kFuse ? 0 : s[1];
        float angle = 0.0f;
        if (kEmit != kFuse) memcpy(&angle, s + 2, 4);
        const orbx_project_item& c = items[b];
        count += quat ? (tree ? emit_one<kEmit, true, true>(c, table, obs, point, octave, angle, level, &r)
                              : emit_one<kEmit, true, false>(c, table, obs, point, octave, angle, level, &r))
                      : (tree ? emit_one<kEmit, false, true>(c, table, obs, point, octave, angle, level, &r)
                              : emit_one<kEmit, false, false>(c, table, obs, point, octave, angle, level, &r));
      }
      memcpy((uint8_t*)out + ((size_t)b * mcap + j) * sizeof(Row), &r, sizeof(Row));
    }
    nvalid[b] = bad ? -1 : count;
  }
}

}  // namespace

struct orbx_project : orbx::side::Handle {};

namespace {

using namespace orbx::side;

// what every form checks before anything is computed, copied or launched; the reason, or nullptr.  `obs` is an argument of last alone
const char* call_problem(const void* points, const void* obs, bool wants_obs, int npoints, const void* items, int nitems, const void* slots,
                         const void* nslots, int mcap, int rot_kind, int sum_order, const void* out, const void* nvalid) {
  if (!points || (wants_obs && !obs) || !items || !slots || !nslots) return "null points, obs, items, slots or nslots";
  if (!out || !nvalid) return "null out or nvalid";
  if (npoints < 1 || nitems < 1 || mcap < 1) return "npoints, nitems and mcap must be at least 1";
  if (const char* e = options_problem(rot_kind, sum_order)) return e;
  if ((long long)nitems * mcap > (long long)INT_MAX) return "nitems * mcap exceeds INT_MAX";
  return nullptr;
}

// the device form of every emitter, after call_problem and the emitter's own checks
template <int kEmit>
int project_device(orbx_project* p, const std::string& who, const void* d_points, const int32_t* d_obs, int npoints, const orbx_project_item* d_items,
                   int nitems, const void* d_slots, const int32_t* d_nslots, int mcap, const float* thresholds, const float* scale_factors,
                   int nlevels, int rot_kind, int sum_order, void* d_out, int32_t* d_nvalid, void* stream) {
  if (((uintptr_t)d_points | (uintptr_t)d_out | (kEmit == kFuse ? 0 : (uintptr_t)d_slots)) & 15)
    return fail(p, ORBX_E_INVALID, who + "d_points, d_slots and d_out must be 16-byte aligned");
  const int chunks = (mcap + kThreads - 1) / kThreads;
  if ((long long)nitems * chunks > (long long)INT_MAX) return fail(p, ORBX_E_INVALID, who + "too many workgroups");
  int rc = same_device(p, who.c_str(), {d_points, d_obs, d_items, d_slots, d_nslots, d_out, d_nvalid}, "the handle");
  if (rc != ORBX_OK) return rc;
  Args g;
  for (int n = 0; n < kMaxT; n++) g.T[n] = (thresholds && n + 1 < nlevels) ? thresholds[n] : INFINITY;
  for (int n = 0; n < kMaxLevels; n++) g.sf[n] = scale_factors ? scale_factors[n < nlevels ? n : nlevels - 1] : 0.0f;
  g.points = (const float4*)d_points; g.obs = d_obs; g.items = d_items; g.slots = d_slots; g.nslots = d_nslots;
  g.out = (float4*)d_out; g.nvalid = d_nvalid;
  g.npoints = npoints; g.nitems = nitems; g.mcap = mcap; g.chunks = chunks; g.stride = kEmit == kFuse ? 1 : 4;
  ORBX_SIDE_HIP(p, hipSetDevice(p->device));
  hipStream_t st = stream ? (hipStream_t)stream : p->st;
  if ((rc = wait_previous(p, st)) != ORBX_OK) return rc;
  hipLaunchKernelGGL(k_project_check, dim3((unsigned)nitems), dim3(kThreads), 0, st, g);
  launch<kEmit>(g, rot_kind, sum_order, st);
  return record_call(p, st);
}

// the host-array form of every emitter: stage, call the device form on the staged copies, read back
template <int kEmit>
int project_host(orbx_project* p, const std::string& who, const orbx_frustum_point* points, const int32_t* obs, int npoints,
                 const orbx_project_item* items, int nitems, const void* slots, const int32_t* nslots, int mcap, const float* thresholds,
                 const float* scale_factors, int nlevels, int rot_kind, int sum_order, void* out, int32_t* nvalid) {
  Stager io;
  const size_t rows = (size_t)nitems * mcap;
  const size_t o_points = io.in(points, (size_t)npoints * sizeof(orbx_frustum_point));
  const size_t o_obs = obs ? io.in(obs, (size_t)npoints * 4) : 0;
  const size_t o_items = io.in(items, (size_t)nitems * sizeof(orbx_project_item));
  const size_t o_slots = io.in(slots, rows * (kEmit == kFuse ? 4 : sizeof(orbx_project_slot))), o_n = io.in(nslots, (size_t)nitems * 4);
  const size_t o_out = io.out(out, rows * sizeof(Row)), o_nvalid = io.out(nvalid, (size_t)nitems * 4);
  int rc = upload(p, io);
  if (rc != ORBX_OK) return rc;
  uint8_t* const d = p->io.p;
  rc = project_device<kEmit>(p, who, d + o_points, obs ? (const int32_t*)(d + o_obs) : nullptr, npoints, (const orbx_project_item*)(d + o_items),
                             nitems, d + o_slots, (const int32_t*)(d + o_n), mcap, thresholds, scale_factors, nlevels, rot_kind, sum_order,
                             d + o_out, (int32_t*)(d + o_nvalid), p->st);
  if (rc != ORBX_OK) return rc;
  return download(p, io);
}

}  // namespace

extern "C" {

int orbx_project_create(orbx_project** out, int device) {
  return create_handle(out, device, "orbx_project_create", orbx_project_destroy, [](orbx_project*) -> const char* { return nullptr; });
}

void orbx_project_destroy(orbx_project* p) { destroy_handle(p); }

const char* orbx_project_last_error(const orbx_project* p) { return last_error(p); }

// ------------------------------------------------------------------------------------------------------------------------------------ last
int orbx_project_last_device(orbx_project* p, const orbx_frustum_point* d_points, const int32_t* d_obs, int npoints,
                             const orbx_project_item* d_items, int nitems, const orbx_project_slot* d_slots, const int32_t* d_nslots, int mcap,
                             int rot_kind, int sum_order, orbx_lastmatch_point* d_out, int32_t* d_nvalid, void* stream) {
  if (!p) return ORBX_E_INVALID;
  const std::string who = "orbx_project_last_device: ";
  if (const char* e = call_problem(d_points, d_obs, true, npoints, d_items, nitems, d_slots, d_nslots, mcap, rot_kind, sum_order, d_out, d_nvalid))
    return fail(p, ORBX_E_INVALID, who + e);
  return project_device<kLast>(p, who, d_points, d_obs, npoints, d_items, nitems, d_slots, d_nslots, mcap, nullptr, nullptr, 1, rot_kind, sum_order,
                               d_out, d_nvalid, stream);
}

int orbx_project_last(orbx_project* p, const orbx_frustum_point* points, const int32_t* obs, int npoints, const orbx_project_item* items, int nitems,
                      const orbx_project_slot* slots, const int32_t* nslots, int mcap, int rot_kind, int sum_order, orbx_lastmatch_point* out,
                      int32_t* nvalid) {
  if (!p) return ORBX_E_INVALID;
  const std::string who = "orbx_project_last: ";
  if (const char* e = call_problem(points, obs, true, npoints, items, nitems, slots, nslots, mcap, rot_kind, sum_order, out, nvalid))
    return fail(p, ORBX_E_INVALID, who + e);
  return project_host<kLast>(p, who, points, obs, npoints, items, nitems, slots, nslots, mcap, nullptr, nullptr, 1, rot_kind, sum_order, out, nvalid);
}

int orbx_project_last_reference(const orbx_frustum_point* points, const int32_t* obs, int npoints, const orbx_project_item* items, int nitems,
                                const orbx_project_slot* slots, const int32_t* nslots, int mcap, int rot_kind, int sum_order,
                                orbx_lastmatch_point* out, int32_t* nvalid) {
  if (const char* e = call_problem(points, obs, true, npoints, items, nitems, slots, nslots, mcap, rot_kind, sum_order, out, nvalid))
    return create_fail(ORBX_E_INVALID, "orbx_project_last_reference", e);
  reference<kLast>(points, obs, npoints, items, nitems, slots, nslots, mcap, HostLevel{1.0f, 1, 0, nullptr}, rot_kind, sum_order, out, nvalid);
  return ORBX_OK;
}

// ----------------------------------------------------------------------------------------------------------------------------------- reloc
int orbx_project_reloc_device(orbx_project* p, const orbx_frustum_point* d_points, int npoints, const orbx_project_item* d_items, int nitems,
                              const orbx_project_slot* d_slots, const int32_t* d_nslots, int mcap, const float* thresholds, int nlevels,
                              int rot_kind, int sum_order, orbx_projmatch_point* d_out, int32_t* d_nvalid, void* stream) {
  if (!p) return ORBX_E_INVALID;
  const std::string who = "orbx_project_reloc_device: ";
  const char* e = call_problem(d_points, nullptr, false, npoints, d_items, nitems, d_slots, d_nslots, mcap, rot_kind, sum_order, d_out, d_nvalid);
  if (!e) e = thresholds_problem(thresholds, nlevels);
  if (e) return fail(p, ORBX_E_INVALID, who + e);
  return project_device<kReloc>(p, who, d_points, nullptr, npoints, d_items, nitems, d_slots, d_nslots, mcap, thresholds, nullptr, nlevels, rot_kind,
                                sum_order, d_out, d_nvalid, stream);
}

int orbx_project_reloc(orbx_project* p, const orbx_frustum_point* points, int npoints, const orbx_project_item* items, int nitems,
                       const orbx_project_slot* slots, const int32_t* nslots, int mcap, const float* thresholds, int nlevels, int rot_kind,
                       int sum_order, orbx_projmatch_point* out, int32_t* nvalid) {
  if (!p) return ORBX_E_INVALID;
  const std::string who = "orbx_project_reloc: ";
  const char* e = call_problem(points, nullptr, false, npoints, items, nitems, slots, nslots, mcap, rot_kind, sum_order, out, nvalid);
  if (!e) e = thresholds_problem(thresholds, nlevels);
  if (e) return fail(p, ORBX_E_INVALID, who + e);
  return project_host<kReloc>(p, who, points, nullptr, npoints, items, nitems, slots, nslots, mcap, thresholds, nullptr, nlevels, rot_kind, sum_order,
                              out, nvalid);
}

int orbx_project_reloc_reference(const orbx_frustum_point* points, int npoints, const orbx_project_item* items, int nitems,
                                 const orbx_project_slot* slots, const int32_t* nslots, int mcap, float log_scale_factor, int nlevels, int log_kind,
                                 int rot_kind, int sum_order, orbx_projmatch_point* out, int32_t* nvalid) {
  const char* e = call_problem(points, nullptr, false, npoints, items, nitems, slots, nslots, mcap, rot_kind, sum_order, out, nvalid);
  if (!e) e = log_problem(log_scale_factor, nlevels, log_kind);
  if (e) return create_fail(ORBX_E_INVALID, "orbx_project_reloc_reference", e);
  reference<kReloc>(points, nullptr, npoints, items, nitems, slots, nslots, mcap, HostLevel{log_scale_factor, nlevels, log_kind, nullptr}, rot_kind,
                    sum_order, out, nvalid);
  return ORBX_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------ fuse
int orbx_project_fuse_device(orbx_project* p, const orbx_frustum_point* d_points, int npoints, const orbx_project_item* d_items, int nitems,
                             const int32_t* d_idx, const int32_t* d_nslots, int mcap, const float* thresholds, const float* scale_factors,
                             int nlevels, int rot_kind, int sum_order, orbx_fuse_query* d_out, int32_t* d_nvalid, void* stream) {
  if (!p) return ORBX_E_INVALID;
  const std::string who = "orbx_project_fuse_device: ";
  const char* e = call_problem(d_points, nullptr, false, npoints, d_items, nitems, d_idx, d_nslots, mcap, rot_kind, sum_order, d_out, d_nvalid);
  if (!e) e = thresholds_problem(thresholds, nlevels);
  if (!e && !scale_factors) e = "null scale_factors";
  if (e) return fail(p, ORBX_E_INVALID, who + e);
  return project_device<kFuse>(p, who, d_points, nullptr, npoints, d_items, nitems, d_idx, d_nslots, mcap, thresholds, scale_factors, nlevels,
                               rot_kind, sum_order, d_out, d_nvalid, stream);
}

int orbx_project_fuse(orbx_project* p, const orbx_frustum_point* points, int npoints, const orbx_project_item* items, int nitems, const int32_t* idx,
                      const int32_t* nslots, int mcap, const float* thresholds, const float* scale_factors, int nlevels, int rot_kind, int sum_order,
                      orbx_fuse_query* out, int32_t* nvalid) {
  if (!p) return ORBX_E_INVALID;
  const std::string who = "orbx_project_fuse: ";
  const char* e = call_problem(points, nullptr, false, npoints, items, nitems, idx, nslots, mcap, rot_kind, sum_order, out, nvalid);
  if (!e) e = thresholds_problem(thresholds, nlevels);
  if (!e && !scale_factors) e = "null scale_factors";
  if (e) return fail(p, ORBX_E_INVALID, who + e);
  return project_host<kFuse>(p, who, points, nullptr, npoints, items, nitems, idx, nslots, mcap, thresholds, scale_factors, nlevels, rot_kind,
                             sum_order, out, nvalid);
}

int orbx_project_fuse_reference(const orbx_frustum_point* points, int npoints, const orbx_project_item* items, int nitems, const int32_t* idx,
                                const int32_t* nslots, int mcap, float log_scale_factor, const float* scale_factors, int nlevels, int log_kind,
                                int rot_kind, int sum_order, orbx_fuse_query* out, int32_t* nvalid) {
  const char* e = call_problem(points, nullptr, false, npoints, items, nitems, idx, nslots, mcap, rot_kind, sum_order, out, nvalid);
  if (!e) e = log_problem(log_scale_factor, nlevels, log_kind);
  if (!e && !scale_factors) e = "null scale_factors";
  if (e) return create_fail(ORBX_E_INVALID, "orbx_project_fuse_reference", e);
  reference<kFuse>(points, nullptr, npoints, items, nitems, idx, nslots, mcap, HostLevel{log_scale_factor, nlevels, log_kind, scale_factors}, rot_kind,
                   sum_order, out, nvalid);
  return ORBX_OK;
}

}  // extern "C"
