// The Sophus Tcw * x projection fronts of SearchByProjection(Frame, LastFrame), the relocalization SearchByProjection and Fuse
// (include/orbx_project.h): B (pose, point list) items over the table of map points liborbx_frustum.so reads, written as the rows the three
// batched matchers read.
//
// emit_one<kEmit, kQuat, kTree> is the specification, stated once for the host and the device; what differs is where the level comes from:
// the host twins call libm's log (HostLevel), the kernel counts the caller's thresholds (DeviceLevel).  Both, sum3, the rigid transform,
// the table's readers, the check, the lanes' bookkeeping, the level checks, the option dispatch and the twins' loop are the projection-front
// core's (../side/orbx_front_device.h, orbx_front_host.h), shared with liborbx_frustum.so and liborbx_sim3.so.
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
#include "../side/orbx_front_host.h"
#include "../../../include/orbx_project.h"

namespace {

using namespace orbx::side::front;
enum { kLast = 0, kReloc = 1, kFuse = 2 };
static_assert(sizeof(orbx_project_slot) == 16, "record sizes");
static_assert(sizeof(orbx_lastmatch_point) == 32 && sizeof(orbx_projmatch_point) == 32 && sizeof(orbx_fuse_query) == 32, "row sizes");

// the skipped row: zero bytes; a fuse query with point = -1
template <int kEmit>
__host__ __device__ inline Row skipped_row() { return {{0u, 0u, 0u, 0u, 0u, 0u, kEmit == kFuse ? 0xFFFFFFFFu : 0u, 0u}}; }

// One slot below nslots with point < npoints (the caller's): the emitter's gates and its row.  Returns whether the row is valid.
template <int kEmit, bool kQuat, bool kTree, class Points, class Level>
__host__ __device__ inline bool emit_one(const orbx_project_item& c, const Points& points, const int32_t* obs_table, int point, int octave,
                                         float angle, const Level& level, Row* r) {
  *r = skipped_row<kEmit>();
  if (point < 0) return false;
  const orbx_frustum_point p = points(point);
  float Pc[3];
  transform<kQuat, kTree>(c.Rcw, c.tcw, c.q, p.pos, Pc);
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

// ---------------------------------------------------------------------------------------------------------------------------- the kernels
struct Args {
  const float4* points; const int32_t* obs; const orbx_project_item* items;
  const int32_t* slots;  // orbx_project_slot rows, or int32 rows (fuse), as their words
  const int32_t* nslots;
  float4* out; int32_t* nvalid;
  int npoints, nitems, mcap, chunks;
  int stride;            // the 32-bit words of one slot: 4 or 1; the point's index is the first
  float T[kMaxT];        // +inf beyond nlevels - 2
  float sf[kMaxLevels];  // fuse: the scale factors, the last repeated beyond nlevels - 1
};

__global__ __launch_bounds__(kThreads) void k_project_check(Args g) {
  const int b = blockIdx.x;
  check_item(g.slots + (size_t)b * g.mcap * g.stride, g.stride, g.nslots[b], g.mcap, g.npoints, false, g.nvalid + b);
}

template <int kEmit, bool kQuat, bool kTree>
__global__ __launch_bounds__(kThreads) void k_project(Args g) {
  const Lane l = lane_of(g.slots, kEmit == kFuse ? 1 : 4, g.nslots, g.nvalid, g.mcap, g.chunks);
  Row r = skipped_row<kEmit>();
  bool valid = false;
  if (l.live) {
    int point = l.point, octave = 0;
    float angle = 0.0f;
    if (kEmit != kFuse) {
      const int4 s = *(const int4*)l.s;
      point = s.x; octave = s.y; angle = __int_as_float(s.z);
    }
    valid = emit_one<kEmit, kQuat, kTree>(g.items[l.b], DevicePoints{g.points}, g.obs, point, octave, angle, DeviceLevel{g.T, g.sf}, &r);
  }
  finish(l, g.out, g.nvalid, r, valid);
}

template <int kEmit>
void launch(const Args& g, int rot_kind, int sum_order, hipStream_t st) {
  dispatch(rot_kind, sum_order, [&](auto q, auto t) {
    hipLaunchKernelGGL((k_project<kEmit, q(), t()>), dim3((unsigned)(g.nitems * g.chunks)), dim3(kThreads), 0, st, g);
  });
}

// the host twin of one emitter
template <int kEmit>
void twin(const orbx_frustum_point* points, const int32_t* obs, int npoints, const orbx_project_item* items, int nitems, const void* slots,
          const int32_t* nslots, int mcap, const HostLevel& level, int rot_kind, int sum_order, void* out, int32_t* nvalid) {
  dispatch(rot_kind, sum_order, [&](auto q, auto t) {
    constexpr bool kQuat = q(), kTree = t();
    reference((const int32_t*)slots, kEmit == kFuse ? 1 : 4, nslots, nitems, mcap, npoints, skipped_row<kEmit>(), out, nvalid,
              [&](int b, const int32_t* s, Row* r) {
                const int octave = kEmit == kFuse ? 0 : s[1];
                float angle = 0.0f;
                if (kEmit != kFuse) memcpy(&angle, s + 2, 4);
                return emit_one<kEmit, kQuat, kTree>(items[b], HostPoints{points}, obs, s[0], octave, angle, level, r);
              });
  });
}

}  // namespace

struct orbx_project : orbx::side::Handle {};

namespace {

using namespace orbx::side;

// what every form checks before anything is computed, copied or launched; the reason, or nullptr.  `obs` is an argument of last alone
const char* call_problem(const void* points, const void* obs, bool wants_obs, int npoints, const void* items, int nitems, const void* slots,
                         const void* nslots, int mcap, int rot_kind, int sum_order, const void* out, const void* nvalid) {
  const char* missing = !points || (wants_obs && !obs) || !items || !slots || !nslots ? "null points, obs, items, slots or nslots"
                        : !out || !nvalid                                               ? "null out or nvalid" : nullptr;
  const char* own = rot_problem(rot_kind);
  return common_problem(missing, npoints, nitems, mcap, own ? own : sum_problem(sum_order));
}

// the device form of every emitter, after call_problem and the emitter's own checks
template <int kEmit>
int project_device(orbx_project* p, const std::string& who, const void* d_points, const int32_t* d_obs, int npoints, const orbx_project_item* d_items,
                   int nitems, const void* d_slots, const int32_t* d_nslots, int mcap, const float* thresholds, const float* scale_factors,
                   int nlevels, int rot_kind, int sum_order, void* d_out, int32_t* d_nvalid, void* stream) {
  int chunks;
  if (const char* e = grid_problem((uintptr_t)d_points | (uintptr_t)d_out | (kEmit == kFuse ? 0 : (uintptr_t)d_slots),
                                   "d_points, d_slots and d_out must be 16-byte aligned", nitems, mcap, &chunks))
    return fail(p, ORBX_E_INVALID, who + e);
  int rc = same_device(p, who.c_str(), {d_points, d_obs, d_items, d_slots, d_nslots, d_out, d_nvalid}, "the handle");
  if (rc != ORBX_OK) return rc;
  Args g;
  fill_levels(g.T, g.sf, thresholds, scale_factors, nlevels);
  g.points = (const float4*)d_points; g.obs = d_obs; g.items = d_items; g.slots = (const int32_t*)d_slots; g.nslots = d_nslots;
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
  twin<kLast>(points, obs, npoints, items, nitems, slots, nslots, mcap, HostLevel{1.0f, 1, 0, nullptr}, rot_kind, sum_order, out, nvalid);
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
  twin<kReloc>(points, nullptr, npoints, items, nitems, slots, nslots, mcap, HostLevel{log_scale_factor, nlevels, log_kind, nullptr}, rot_kind,
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
  twin<kFuse>(points, nullptr, npoints, items, nitems, idx, nslots, mcap, HostLevel{log_scale_factor, nlevels, log_kind, scale_factors}, rot_kind,
                   sum_order, out, nvalid);
  return ORBX_OK;
}

}  // extern "C"
