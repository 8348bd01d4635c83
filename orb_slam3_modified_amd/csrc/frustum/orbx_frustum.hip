// The batched Frame::isInFrustum + MapPoint::PredictScale (include/orbx_frustum.h): B (pose, local map) items over a table of map points in
// HBM, written as the orbx_localmatch_point rows the batched SearchLocalPoints reads.
//
// project_one<kTree> is the specification, stated once for the host and the device; what differs is where the level comes from: the host
// twin calls libm's log (HostLevel), the kernel counts the thresholds the host bisected through that same libm (DeviceLevel).  Both, the
// bisection, sum3, the table's readers, the check and the lanes' bookkeeping are the projection-front core's (../side/orbx_front_device.h,
// orbx_front_host.h), shared with liborbx_project.so and liborbx_sim3.so.
//
// k_frustum_check      one workgroup per item: nmp and every index of the row's first nmp against npoints, before any of them addresses the
//                      table; d_ntomatch[b] = -1 (malformed) or 0.
// k_frustum<kTree>     a lane per (item, slot), 256 slots a workgroup, the workgroups of one item consecutive: the item is wave-uniform,
//                      so its 25 constants come through scalar loads from d_items[b] and the thresholds from the kernel arguments.  A lane
//                      gathers its 48-byte record in 16-byte loads (of the third only max_dist is fetched: the rest is padding) and writes
//                      its 32-byte record as two 16-byte stores.  ntomatch: a
//                      ballot and a popcount per wave, one integer atomic add per wave that counted anything.
// The float expressions are compiled with -ffp-contract=off and hipcc's correctly rounded fp32 divide and sqrt; no fast-math flag.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "../side/orbx_handle.h"
#include "../side/orbx_front_host.h"
#include "../../../include/orbx_frustum.h"

namespace {

using namespace orbx::side::front;
static_assert(sizeof(orbx_frustum_item) == 112 && sizeof(orbx_localmatch_point) == 32, "record sizes");

// Steps 1 .. 11 of the header for one slot below nmp; idx < npoints is the caller's.  Returns whether the slot counts in ntomatch.
template <bool kTree, class Points, class Level>
__host__ __device__ inline bool project_one(const orbx_frustum_item& c, const Points& points, const int32_t* obs_table, int idx, float cos_limit,
                                            const Level& level, orbx_localmatch_point* r, float* depth) {
  *r = {-1.0f, -1.0f, 0.0f, 0.0f, 0, 0, idx, 0};
  *depth = 0.0f;
  if (idx < 0) return false;
  const int obs = obs_table[idx];
  if (obs < 0) return false;
  const orbx_frustum_point p = points(idx);
  float Pc[3];
  for (int k = 0; k < 3; k++) Pc[k] = sum3<kTree>(c.Rcw[3 * k] * p.pos[0], c.Rcw[3 * k + 1] * p.pos[1], c.Rcw[3 * k + 2] * p.pos[2]) + c.tcw[k];
  const float Pc_dist = sqrtf(sum3<kTree>(Pc[0] * Pc[0], Pc[1] * Pc[1], Pc[2] * Pc[2]));
  const float invz = 1.0f / Pc[2];
  if (Pc[2] < 0.0f) return false;
  const float u = (c.fx * Pc[0]) / Pc[2] + c.cx, v = (c.fy * Pc[1]) / Pc[2] + c.cy;
  if (u < c.bounds[0] || u > c.bounds[2]) return false;
  if (v < c.bounds[1] || v > c.bounds[3]) return false;
  r->proj_x = u; r->proj_y = v;
  const float PO[3] = {p.pos[0] - c.Ow[0], p.pos[1] - c.Ow[1], p.pos[2] - c.Ow[2]};
  const float dist = sqrtf(sum3<kTree>(PO[0] * PO[0], PO[1] * PO[1], PO[2] * PO[2]));
  if (dist < p.min_inv || dist > p.max_inv) return false;
  const float viewCos = sum3<kTree>(PO[0] * p.normal[0], PO[1] * p.normal[1], PO[2] * p.normal[2]) / dist;
  if (viewCos < cos_limit) return false;
  const float ratio = p.max_dist / dist;
  const float prod = c.mbf * invz;
  r->proj_xr = u - prod;
  r->view_cos = viewCos;
  r->level = level(ratio);
  r->obs = obs;
  r->in_view = (c.far_th > 0.0f && Pc_dist > c.far_th) ? 0 : 1;
  *depth = Pc_dist;
  return true;
}

const char* options_problem(int nlevels, int sum_order, int log_kind) {
  if (const char* e = levels_problem(nlevels)) return e;
  if (const char* e = sum_problem(sum_order)) return e;
  if (log_kind != ORBX_FRUSTUM_LOG_DOUBLE && log_kind != ORBX_FRUSTUM_LOG_FLOAT) return "unknown log_kind";
  return nullptr;
}

// ---------------------------------------------------------------------------------------------------------------------------- the kernels
struct Args {
  const float4* points; const int32_t* obs; const orbx_frustum_item* items; const int32_t* idx; const int32_t* nmp;
  float4* mp; float* depth; int32_t* ntomatch;
  int npoints, nitems, mcap, chunks;
  int all_bad;           // the call's log_scale_factor is not finite and positive
  float cos_limit;
  float T[kMaxT];        // +inf beyond nlevels - 2
};

__global__ __launch_bounds__(kThreads) void k_frustum_check(Args g) {
  const int b = blockIdx.x;
  check_item(g.idx + (size_t)b * g.mcap, 1, g.nmp[b], g.mcap, g.npoints, g.all_bad, g.ntomatch + b);
}

template <bool kTree>
__global__ __launch_bounds__(kThreads) void k_frustum(Args g) {
  const Lane l = lane_of(g.idx, 1, g.nmp, g.ntomatch, g.mcap, g.chunks);
  orbx_localmatch_point r = {0.0f, 0.0f, 0.0f, 0.0f, 0, 0, 0, 0};
  float depth = 0.0f;
  bool counts = false;
  if (l.live) counts = project_one<kTree>(g.items[l.b], DevicePoints{g.points}, g.obs, l.point, g.cos_limit, DeviceLevel{g.T, nullptr}, &r, &depth);
  finish(l, g.mp, g.ntomatch, Row{{fw(r.proj_x), fw(r.proj_y), fw(r.proj_xr), fw(r.view_cos), iw(r.level), iw(r.obs), iw(r.point), iw(r.in_view)}}, counts,
         g.depth, depth);
}

}  // namespace

struct orbx_frustum : orbx::side::Handle {   // the thresholds of the last (log_scale_factor, nlevels, log_kind)
  bool have = false;
  uint32_t lsf_bits = 0;
  int nlevels = 0, log_kind = 0;
  float T[kMaxT];
};

namespace {

using namespace orbx::side;

// what every form checks before anything is computed, copied or launched; the reason, or nullptr
const char* call_problem(const void* points, const void* obs, int npoints, const void* items, int nitems, const void* idx, const void* nmp, int mcap,
                         int nlevels, float cos_limit, int sum_order, int log_kind, const void* mp, const void* ntomatch) {
  const char* missing = !points || !obs || !items || !idx || !nmp ? "null points, obs, items, idx or nmp" : !mp || !ntomatch ? "null mp or ntomatch" : nullptr;
  const char* own = options_problem(nlevels, sum_order, log_kind);
  if (!own && cos_limit != cos_limit) own = "cos_limit is NaN";
  return common_problem(missing, npoints, nitems, mcap, own);
}

}  // namespace

extern "C" {

int orbx_frustum_create(orbx_frustum** out, int device) {
  return create_handle(out, device, "orbx_frustum_create", orbx_frustum_destroy, [](orbx_frustum*) -> const char* { return nullptr; });
}

void orbx_frustum_destroy(orbx_frustum* f) { destroy_handle(f); }

const char* orbx_frustum_last_error(const orbx_frustum* f) { return last_error(f); }

int orbx_frustum_level_thresholds(float log_scale_factor, int nlevels, int log_kind, float* thresholds) {
  const char* who = "orbx_frustum_level_thresholds";
  if (const char* e = options_problem(nlevels, ORBX_FRUSTUM_SUM_LTR, log_kind)) return create_fail(ORBX_E_INVALID, who, e);
  if (!thresholds && nlevels > 1) return create_fail(ORBX_E_INVALID, who, "null thresholds");
  if (!usable_lsf(log_scale_factor)) return create_fail(ORBX_E_INVALID, who, "log_scale_factor must be finite and positive");
  float T[kMaxT];
  std::string why;
  if (const char* e = level_thresholds(log_scale_factor, nlevels, log_kind, T, &why)) return create_fail(ORBX_E_INVALID, who, e);
  for (int n = 0; n + 1 < nlevels; n++) thresholds[n] = T[n];
  return ORBX_OK;
}

int orbx_frustum_project_device(orbx_frustum* f, const orbx_frustum_point* d_points, const int32_t* d_obs, int npoints,
                                const orbx_frustum_item* d_items, int nitems, const int32_t* d_idx, const int32_t* d_nmp, int mcap,
                                float log_scale_factor, int nlevels, float cos_limit, int sum_order, int log_kind, orbx_localmatch_point* d_mp,
                                float* d_depth, int32_t* d_ntomatch, void* stream) {
  if (!f) return ORBX_E_INVALID;
  const std::string who = "orbx_frustum_project_device: ";
  if (const char* e = call_problem(d_points, d_obs, npoints, d_items, nitems, d_idx, d_nmp, mcap, nlevels, cos_limit, sum_order, log_kind, d_mp,
                                   d_ntomatch))
    return fail(f, ORBX_E_INVALID, who + e);
  int chunks;
  if (const char* e = grid_problem((uintptr_t)d_points | (uintptr_t)d_mp, "d_points and d_mp must be 16-byte aligned", nitems, mcap, &chunks))
    return fail(f, ORBX_E_INVALID, who + e);
  int rc = same_device(f, who.c_str(), {d_points, d_obs, d_items, d_idx, d_nmp, d_mp, d_depth, d_ntomatch}, "the handle");
  if (rc != ORBX_OK) return rc;
  Args g;
  g.all_bad = !usable_lsf(log_scale_factor);
  if (!g.all_bad) {
    uint32_t bits;
    memcpy(&bits, &log_scale_factor, 4);
    if (!(f->have && f->lsf_bits == bits && f->nlevels == nlevels && f->log_kind == log_kind)) {
      std::string why;
      f->have = false;
      if (const char* e = level_thresholds(log_scale_factor, nlevels, log_kind, f->T, &why)) return fail(f, ORBX_E_INVALID, who + e);
      f->have = true; f->lsf_bits = bits; f->nlevels = nlevels; f->log_kind = log_kind;
    }
  }
  fill_levels(g.T, nullptr, g.all_bad ? nullptr : f->T, nullptr, nlevels);
  g.points = (const float4*)d_points; g.obs = d_obs; g.items = d_items; g.idx = d_idx; g.nmp = d_nmp;
  g.mp = (float4*)d_mp; g.depth = d_depth; g.ntomatch = d_ntomatch;
  g.npoints = npoints; g.nitems = nitems; g.mcap = mcap; g.chunks = chunks; g.cos_limit = cos_limit;
  ORBX_SIDE_HIP(f, hipSetDevice(f->device));
  hipStream_t st = stream ? (hipStream_t)stream : f->st;
  if ((rc = wait_previous(f, st)) != ORBX_OK) return rc;
  hipLaunchKernelGGL(k_frustum_check, dim3((unsigned)nitems), dim3(kThreads), 0, st, g);
  const dim3 grid((unsigned)(nitems * chunks));
  if (sum_order == ORBX_FRUSTUM_SUM_TREE) hipLaunchKernelGGL(k_frustum<true>, grid, dim3(kThreads), 0, st, g);
  else hipLaunchKernelGGL(k_frustum<false>, grid, dim3(kThreads), 0, st, g);
  return record_call(f, st);
}

int orbx_frustum_project(orbx_frustum* f, const orbx_frustum_point* points, const int32_t* obs, int npoints, const orbx_frustum_item* items,
                         int nitems, const int32_t* idx, const int32_t* nmp, int mcap, float log_scale_factor, int nlevels, float cos_limit,
                         int sum_order, int log_kind, orbx_localmatch_point* mp, float* depth, int32_t* ntomatch) {
  if (!f) return ORBX_E_INVALID;
  const std::string who = "orbx_frustum_project: ";
  if (const char* e = call_problem(points, obs, npoints, items, nitems, idx, nmp, mcap, nlevels, cos_limit, sum_order, log_kind, mp, ntomatch))
    return fail(f, ORBX_E_INVALID, who + e);
  Stager io;
  const size_t slots = (size_t)nitems * mcap;
  const size_t o_points = io.in(points, (size_t)npoints * sizeof(orbx_frustum_point)), o_obs = io.in(obs, (size_t)npoints * 4);
  const size_t o_items = io.in(items, (size_t)nitems * sizeof(orbx_frustum_item)), o_idx = io.in(idx, slots * 4), o_nmp = io.in(nmp, (size_t)nitems * 4);
  const size_t o_mp = io.out(mp, slots * sizeof(orbx_localmatch_point)), o_depth = io.out(depth, slots * 4), o_n = io.out(ntomatch, (size_t)nitems * 4);
  int rc = upload(f, io);
  if (rc != ORBX_OK) return rc;
  uint8_t* const d = f->io.p;
  rc = orbx_frustum_project_device(f, (const orbx_frustum_point*)(d + o_points), (const int32_t*)(d + o_obs), npoints,
                                   (const orbx_frustum_item*)(d + o_items), nitems, (const int32_t*)(d + o_idx), (const int32_t*)(d + o_nmp), mcap,
                                   log_scale_factor, nlevels, cos_limit, sum_order, log_kind, (orbx_localmatch_point*)(d + o_mp),
                                   depth ? (float*)(d + o_depth) : nullptr, (int32_t*)(d + o_n), f->st);
  if (rc != ORBX_OK) return rc;
  return download(f, io);
}

int orbx_frustum_project_reference(const orbx_frustum_point* points, const int32_t* obs, int npoints, const orbx_frustum_item* items, int nitems,
                                   const int32_t* idx, const int32_t* nmp, int mcap, float log_scale_factor, int nlevels, float cos_limit,
                                   int sum_order, int log_kind, orbx_localmatch_point* mp, float* depth, int32_t* ntomatch) {
  if (const char* e = call_problem(points, obs, npoints, items, nitems, idx, nmp, mcap, nlevels, cos_limit, sum_order, log_kind, mp, ntomatch))
    return create_fail(ORBX_E_INVALID, "orbx_frustum_project_reference", e);
  const HostLevel level = {log_scale_factor, nlevels, log_kind, nullptr};
  const HostPoints table = {points};
  const bool all_bad = !usable_lsf(log_scale_factor);
  for (int b = 0; b < nitems; b++) {
    const int32_t* row = idx + (size_t)b * mcap;
    bool bad = all_bad || nmp[b] < 0 || nmp[b] > mcap;
    for (int j = 0; !bad && j < nmp[b]; j++) bad = row[j] >= npoints;
    const int n = bad ? 0 : nmp[b];
    int count = 0;
    for (int j = 0; j < mcap; j++) {
      const size_t slot = (size_t)b * mcap + j;
      orbx_localmatch_point r = {0.0f, 0.0f, 0.0f, 0.0f, 0, 0, 0, 0};
      float dep = 0.0f;
      if (j < n)
        count += sum_order == ORBX_FRUSTUM_SUM_TREE ? project_one<true>(items[b], table, obs, row[j], cos_limit, level, &r, &dep)
                                                    : project_one<false>(items[b], table, obs, row[j], cos_limit, level, &r, &dep);
      mp[slot] = r;
      if (depth) depth[slot] = dep;
    }
    ntomatch[b] = bad ? -1 : count;
  }
  return ORBX_OK;
}

}  // extern "C"
