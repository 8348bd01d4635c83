// The projection fronts of LoopClosing's matcher callers (the two Sim3 SearchByProjection overloads, the Sim3 Fuse, both directions of
// SearchBySim3) and SearchBySim3's agreement pass (include/orbx_sim3.h): B items over the table of map points liborbx_frustum.so reads,
// written as the rows liborbx_projmatch.so and liborbx_fuse.so read.
//
// emit_pose<kEmit, kQuat, kTree> (proj in its two forms, fuse) and emit_search<kQuat, kTree, kSimQuat> are the specification, each stated
// once for the host and the device; what differs is where the level comes from: the host twins call libm's log (HostLevel), the kernels
// count the caller's thresholds (DeviceLevel).  Both, sum3, the rigid transform, the table's readers, the check, the lanes' bookkeeping, the
// level checks, the option dispatch and the twins' loop are the projection-front core's (../side/orbx_front_device.h, orbx_front_host.h),
// shared with liborbx_frustum.so and liborbx_project.so.
//
// k_sim3_check               one workgroup per item: nslots and every index of the row's first nslots against npoints, before any of them
//                            addresses the table; d_nvalid[b] = -1 (malformed) or 0.
// k_sim3_pose<kEmit, ...>    a lane per (item, slot), 256 slots a workgroup, the workgroups of one item consecutive: the item is
// k_sim3_search<...>         workgroup-uniform, so its constants come through scalar loads from d_items[b], the thresholds and the scale
//                            factors from the kernel arguments.  A lane reads its index, gathers what its emitter needs of the 48-byte
//                            record in 16-byte loads and writes its 32-byte row as two 16-byte stores.  nvalid: a ballot and a popcount per
//                            wave, one integer atomic add per wave that counted anything.
// k_sim3_agree_check         a lane per pair: the two input counts and n1, n2 against qcap; d_nfound[p] = -1 or 0.
// k_sim3_agree               a lane per (pair, i1): integer compares, one checked gather from the 21 blocks, the count as above.
// The float expressions are compiled with -ffp-contract=off and hipcc's correctly rounded fp32 divide and sqrt; no fast-math flag.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>

#include "../side/orbx_handle.h"
#include "../side/orbx_front_host.h"
#include "../../../include/orbx_sim3.h"

namespace {

using namespace orbx::side::front;
enum { kProj = 0, kFuse = 1, kSearch = 2, kProjKfs = 3 };   // kProjKfs: the vpPointsKFs overload, which projects as SearchBySim3 does
static_assert(sizeof(orbx_sim3_item) == 176, "record sizes");
static_assert(sizeof(orbx_projmatch_point) == 32 && sizeof(orbx_fuse_query) == 32, "row sizes");

// the skipped row: zero bytes; a query with point = -1
template <int kEmit>
__host__ __device__ inline Row skipped_row() { return {{0u, 0u, 0u, 0u, 0u, 0u, kEmit == kProj || kEmit == kProjKfs ? 0u : 0xFFFFFFFFu, 0u}}; }

// Pb = S * Pa for a similarity (s, R, t, the RxSO3's quaternion q)
template <bool kSimQuat, bool kTree>
__host__ __device__ inline void similarity(float s, const float* R, const float* t, const float* q, const float* Pa, float* Pb) {
  if (kSimQuat) {
    float uv[3], x[3];
    cross3(q, Pa, uv);
    for (int k = 0; k < 3; k++) uv[k] = uv[k] + uv[k];
    cross3(q, uv, x);
    for (int k = 0; k < 3; k++) Pb[k] = (s * Pa[k] + (q[3] * uv[k] + x[k])) + t[k];
  } else {
    for (int k = 0; k < 3; k++) Pb[k] = (sum3<kTree>(R[3 * k] * Pa[0], R[3 * k + 1] * Pa[1], R[3 * k + 2] * Pa[2]) * s) + t[k];
  }
}

// proj and fuse: one slot below nslots with point < npoints (the caller's).  Returns whether the row is valid.
template <int kEmit, bool kQuat, bool kTree, class Points, class Level>
__host__ __device__ inline bool emit_pose(const orbx_project_item& c, const Points& points, int point, const Level& level, Row* r) {
  *r = skipped_row<kEmit>();
  if (point < 0) return false;
  const orbx_frustum_point p = points(point);
  float Pc[3];
  transform<kQuat, kTree>(c.Rcw, c.tcw, c.q, p.pos, Pc);
  if (kEmit == kFuse) {
    if (Pc[2] < 0.0f) return false;
  } else {
    if ((double)Pc[2] < 0.0) return false;
  }
  float u, v;
  if (kEmit == kProjKfs) {   // :573-578: invz = 1 / z, x = X * invz, u = fx * x + cx
    const float invz = 1.0f / Pc[2];
    const float x = Pc[0] * invz, y = Pc[1] * invz;
    u = c.fx * x + c.cx;
    v = c.fy * y + c.cy;
  } else {                   // Pinhole::project (:465, :1379) divides by z
    u = (c.fx * Pc[0]) / Pc[2] + c.cx;
    v = (c.fy * Pc[1]) / Pc[2] + c.cy;
  }
  if (!(u >= c.bounds[0] && u < c.bounds[2])) return false;   // KeyFrame::IsInImage: half-open, a NaN fails
  if (!(v >= c.bounds[1] && v < c.bounds[3])) return false;
  const float PO[3] = {p.pos[0] - c.Ow[0], p.pos[1] - c.Ow[1], p.pos[2] - c.Ow[2]};
  const float dist = sqrtf(sum3<kTree>(PO[0] * PO[0], PO[1] * PO[1], PO[2] * PO[2]));
  if (dist < p.min_inv || dist > p.max_inv) return false;
  const float dot = sum3<kTree>(PO[0] * p.normal[0], PO[1] * p.normal[1], PO[2] * p.normal[2]);
  if ((double)dot < 0.5 * (double)dist) return false;
  const float ratio = p.max_dist / dist;
  int lvl;
  float scale;
  level(ratio, &lvl, &scale);
  if (kEmit != kFuse) {
    *r = {{fw(u), fw(v), fw(0.0f), iw(lvl), iw(point), 1u, 0u, 0u}};
  } else {
    const float radius = c.th * scale;
    *r = {{fw(u), fw(v), fw(radius), fw(0.0f), iw(lvl - 1), iw(lvl), iw(point), 0u}};
  }
  return true;
}

// search: one slot of one direction of SearchBySim3
template <bool kQuat, bool kTree, bool kSimQuat, class Points, class Level>
__host__ __device__ inline bool emit_search(const orbx_sim3_item& c, const Points& points, int point, const Level& level, Row* r) {
  *r = skipped_row<kSearch>();
  if (point < 0) return false;
  const orbx_frustum_point p = points(point);
  float Pa[3], Pb[3];
  transform<kQuat, kTree>(c.Raw, c.taw, c.qa, p.pos, Pa);
  similarity<kSimQuat, kTree>(c.s, c.Rba, c.tba, c.qba, Pa, Pb);
  if ((double)Pb[2] < 0.0) return false;
  const float invz = 1.0f / Pb[2];
  const float x = Pb[0] * invz, y = Pb[1] * invz;
  const float u = c.fx * x + c.cx, v = c.fy * y + c.cy;
  if (!(u >= c.bounds[0] && u < c.bounds[2])) return false;
  if (!(v >= c.bounds[1] && v < c.bounds[3])) return false;
  const float dist = sqrtf(sum3<kTree>(Pb[0] * Pb[0], Pb[1] * Pb[1], Pb[2] * Pb[2]));
  if (dist < p.min_inv || dist > p.max_inv) return false;
  const float ratio = p.max_dist / dist;
  int lvl;
  float scale;
  level(ratio, &lvl, &scale);
  const float radius = c.th * scale;
  *r = {{fw(u), fw(v), fw(radius), fw(0.0f), iw(lvl - 1), iw(lvl), iw(point), 0u}};
  return true;
}

// agree: the entry of match12 for keypoint i1 < n1 of a sound pair; gather(idx2) = vnMatch2[idx2], called for 0 <= idx2 < n2 only
template <class Gather>
__host__ __device__ inline int agree_one(int i1, int best_idx12, int best_dist12, int n2, int th_high, const Gather& vn_match2) {
  const int idx2 = best_dist12 <= th_high ? best_idx12 : -1;
  if (idx2 < 0 || idx2 >= n2) return -1;
  return vn_match2(idx2) == i1 ? idx2 : -1;
}
__host__ __device__ inline bool pair_is_bad(int nfound12, int nfound21, int n1, int n2, int qcap) {
  return nfound12 < 0 || nfound21 < 0 || n1 < 0 || n1 > qcap || n2 < 0 || n2 > qcap;
}
struct Match2 {   // vnMatch2 of one pair
  const int32_t* idx; const int32_t* dist; int th_high;
  __host__ __device__ int operator()(int i2) const { return dist[i2] <= th_high ? idx[i2] : -1; }
};

const char* proj_problem(int proj_kind) {
  return proj_kind != ORBX_SIM3_PROJ_DIVIDE && proj_kind != ORBX_SIM3_PROJ_INVZ ? "unknown proj_kind" : nullptr;
}
const char* options_problem(int rot_kind, int sum_order, int sim_kind) {
  if (const char* e = rot_problem(rot_kind)) return e;
  if (const char* e = sum_problem(sum_order)) return e;
  if (sim_kind != ORBX_SIM3_MATRIX && sim_kind != ORBX_SIM3_QUAT) return "unknown sim_kind";
  return nullptr;
}

// ---------------------------------------------------------------------------------------------------------------------------- the kernels
struct Args {
  const float4* points;
  const void* items;     // orbx_project_item (proj, fuse) or orbx_sim3_item (search)
  const int32_t* idx; const int32_t* nslots;
  float4* out; int32_t* nvalid;
  int npoints, nitems, mcap, chunks;
  float T[kMaxT];        // +inf beyond nlevels - 2
  float sf[kMaxLevels];  // the scale factors, the last repeated beyond nlevels - 1 (proj: zeros, not read)
};

__global__ __launch_bounds__(kThreads) void k_sim3_check(Args g) {
  const int b = blockIdx.x;
  check_item(g.idx + (size_t)b * g.mcap, 1, g.nslots[b], g.mcap, g.npoints, false, g.nvalid + b);
}

template <int kEmit, bool kQuat, bool kTree>
__global__ __launch_bounds__(kThreads) void k_sim3_pose(Args g) {
  const Lane l = lane_of(g.idx, 1, g.nslots, g.nvalid, g.mcap, g.chunks);
  Row r = skipped_row<kEmit>();
  bool valid = false;
  if (l.live) valid = emit_pose<kEmit, kQuat, kTree>(((const orbx_project_item*)g.items)[l.b], DevicePoints{g.points}, l.point, DeviceLevel{g.T, g.sf}, &r);
  finish(l, g.out, g.nvalid, r, valid);
}

template <bool kQuat, bool kTree, bool kSimQuat>
__global__ __launch_bounds__(kThreads) void k_sim3_search(Args g) {
  const Lane l = lane_of(g.idx, 1, g.nslots, g.nvalid, g.mcap, g.chunks);
  Row r = skipped_row<kSearch>();
  bool valid = false;
  if (l.live) valid = emit_search<kQuat, kTree, kSimQuat>(((const orbx_sim3_item*)g.items)[l.b], DevicePoints{g.points}, l.point, DeviceLevel{g.T, g.sf}, &r);
  finish(l, g.out, g.nvalid, r, valid);
}

template <int kEmit>
void launch(const Args& g, int rot_kind, int sum_order, int sim_kind, hipStream_t st) {
  const dim3 grid((unsigned)(g.nitems * g.chunks)), block(kThreads);
  dispatch(rot_kind, sum_order, [&](auto q, auto t) {
    constexpr bool kQuat = q(), kTree = t();
    if constexpr (kEmit != kSearch) hipLaunchKernelGGL((k_sim3_pose<kEmit, kQuat, kTree>), grid, block, 0, st, g);
    else pick(sim_kind == ORBX_SIM3_QUAT, [&](auto s) { hipLaunchKernelGGL((k_sim3_search<kQuat, kTree, s()>), grid, block, 0, st, g); });
  });
}

struct AgreeArgs {
  const int32_t* idx12; const int32_t* dist12; const int32_t* nf12;
  const int32_t* idx21; const int32_t* dist21; const int32_t* nf21;
  const int32_t* n1; const int32_t* n2;
  int32_t* match12; int32_t* nfound;
  int npairs, qcap, chunks, th_high;
};

__global__ __launch_bounds__(kThreads) void k_sim3_agree_check(AgreeArgs g) {
  const int p = (int)(blockIdx.x * kThreads + threadIdx.x);
  if (p < g.npairs) g.nfound[p] = pair_is_bad(g.nf12[p], g.nf21[p], g.n1[p], g.n2[p], g.qcap) ? -1 : 0;
}

__global__ __launch_bounds__(kThreads) void k_sim3_agree(AgreeArgs g) {
  const int p = (int)(blockIdx.x / (unsigned)g.chunks);
  const int i1 = (int)(blockIdx.x - (unsigned)p * (unsigned)g.chunks) * kThreads + (int)threadIdx.x;
  const bool bad = __hip_atomic_load(g.nfound + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0;
  const int n1 = bad ? 0 : g.n1[p], n2 = bad ? 0 : g.n2[p];   // both within 0 .. qcap
  const size_t row = (size_t)p * g.qcap;
  int m = -1;
  if (i1 < n1) m = agree_one(i1, g.idx12[row + i1], g.dist12[row + i1], n2, g.th_high, Match2{g.idx21 + row, g.dist21 + row, g.th_high});
  if (i1 < g.qcap) g.match12[row + i1] = m;
  const int count = __popcll(__ballot(m >= 0));
  if (count > 0 && (threadIdx.x & 63) == 0) atomicAdd(g.nfound + p, count);
}

// the host twin of one emitter
template <int kEmit>
void twin(const orbx_frustum_point* points, int npoints, const void* items, int nitems, const int32_t* idx, const int32_t* nslots, int mcap,
          const HostLevel& level, int rot_kind, int sum_order, int sim_kind, void* out, int32_t* nvalid) {
  const HostPoints table = {points};
  dispatch(rot_kind, sum_order, [&](auto q, auto t) {
    constexpr bool kQuat = q(), kTree = t();
    auto loop = [&](auto emit) { reference(idx, 1, nslots, nitems, mcap, npoints, skipped_row<kEmit>(), out, nvalid, emit); };
    if constexpr (kEmit != kSearch)
      loop([&](int b, const int32_t* s, Row* r) { return emit_pose<kEmit, kQuat, kTree>(((const orbx_project_item*)items)[b], table, s[0], level, r); });
    else
      pick(sim_kind == ORBX_SIM3_QUAT, [&](auto sq) {
        constexpr bool kSimQuat = sq();
        loop([&](int b, const int32_t* s, Row* r) { return emit_search<kQuat, kTree, kSimQuat>(((const orbx_sim3_item*)items)[b], table, s[0], level, r); });
      });
  });
}

}  // namespace

struct orbx_sim3 : orbx::side::Handle {};

namespace {

using namespace orbx::side;

// what every emitter form checks before anything is computed, copied or launched; the reason, or nullptr
const char* call_problem(const void* points, int npoints, const void* items, int nitems, const void* idx, const void* nslots, int mcap, int rot_kind,
                         int sum_order, int sim_kind, const void* out, const void* nvalid) {
  const char* missing = !points || !items || !idx || !nslots ? "null points, items, idx or nslots" : !out || !nvalid ? "null out or nvalid" : nullptr;
  return common_problem(missing, npoints, nitems, mcap, options_problem(rot_kind, sum_order, sim_kind));
}
// ... and what the three forms of agree check
const char* agree_problem(const void* i12, const void* d12, const void* f12, const void* i21, const void* d21, const void* f21, const void* n1,
                          const void* n2, int npairs, int qcap, const void* match12, const void* nfound) {
  if (!i12 || !d12 || !f12 || !i21 || !d21 || !f21 || !n1 || !n2) return "null best_idx, best_dist, nfound, n1 or n2";
  if (!match12 || !nfound) return "null match12 or nfound";
  if (npairs < 1 || qcap < 1) return "npairs and qcap must be at least 1";
  if ((long long)npairs * qcap > (long long)INT_MAX) return "npairs * qcap exceeds INT_MAX";
  return nullptr;
}

// the device form of every emitter, after call_problem and the emitter's own checks
template <int kEmit>
int emit_device(orbx_sim3* p, const std::string& who, const void* d_points, int npoints, const void* d_items, int nitems, const int32_t* d_idx,
                const int32_t* d_nslots, int mcap, const float* thresholds, const float* scale_factors, int nlevels, int rot_kind, int sum_order,
                int sim_kind, void* d_out, int32_t* d_nvalid, void* stream) {
  int chunks;
  if (const char* e = grid_problem((uintptr_t)d_points | (uintptr_t)d_out | (uintptr_t)d_items, "d_points, d_items and d_out must be 16-byte aligned",
                                   nitems, mcap, &chunks))
    return fail(p, ORBX_E_INVALID, who + e);
  int rc = same_device(p, who.c_str(), {d_points, d_items, d_idx, d_nslots, d_out, d_nvalid}, "the handle");
  if (rc != ORBX_OK) return rc;
  Args g;
  fill_levels(g.T, g.sf, thresholds, scale_factors, nlevels);
  g.points = (const float4*)d_points; g.items = d_items; g.idx = d_idx; g.nslots = d_nslots;
  g.out = (float4*)d_out; g.nvalid = d_nvalid;
  g.npoints = npoints; g.nitems = nitems; g.mcap = mcap; g.chunks = chunks;
  ORBX_SIDE_HIP(p, hipSetDevice(p->device));
  hipStream_t st = stream ? (hipStream_t)stream : p->st;
  if ((rc = wait_previous(p, st)) != ORBX_OK) return rc;
  hipLaunchKernelGGL(k_sim3_check, dim3((unsigned)nitems), dim3(kThreads), 0, st, g);
  launch<kEmit>(g, rot_kind, sum_order, sim_kind, st);
  return record_call(p, st);
}

// the host-array form of every emitter: stage, call the device form on the staged copies, read back
template <int kEmit>
int emit_host(orbx_sim3* p, const std::string& who, const orbx_frustum_point* points, int npoints, const void* items, int nitems, const int32_t* idx,
              const int32_t* nslots, int mcap, const float* thresholds, const float* scale_factors, int nlevels, int rot_kind, int sum_order,
              int sim_kind, void* out, int32_t* nvalid) {
  Stager io;
  const size_t rows = (size_t)nitems * mcap;
  const size_t o_points = io.in(points, (size_t)npoints * sizeof(orbx_frustum_point));
  const size_t o_items = io.in(items, (size_t)nitems * (kEmit == kSearch ? sizeof(orbx_sim3_item) : sizeof(orbx_project_item)));
  const size_t o_idx = io.in(idx, rows * 4), o_n = io.in(nslots, (size_t)nitems * 4);
  const size_t o_out = io.out(out, rows * sizeof(Row)), o_nvalid = io.out(nvalid, (size_t)nitems * 4);
  int rc = upload(p, io);
  if (rc != ORBX_OK) return rc;
  uint8_t* const d = p->io.p;
  rc = emit_device<kEmit>(p, who, d + o_points, npoints, d + o_items, nitems, (const int32_t*)(d + o_idx), (const int32_t*)(d + o_n), mcap, thresholds,
                          scale_factors, nlevels, rot_kind, sum_order, sim_kind, d + o_out, (int32_t*)(d + o_nvalid), p->st);
  if (rc != ORBX_OK) return rc;
  return download(p, io);
}

}  // namespace

extern "C" {

int orbx_sim3_create(orbx_sim3** out, int device) {
  return create_handle(out, device, "orbx_sim3_create", orbx_sim3_destroy, [](orbx_sim3*) -> const char* { return nullptr; });
}

void orbx_sim3_destroy(orbx_sim3* p) { destroy_handle(p); }

const char* orbx_sim3_last_error(const orbx_sim3* p) { return last_error(p); }

// ------------------------------------------------------------------------------------------------------------------------------------ proj
int orbx_sim3_proj_device(orbx_sim3* p, const orbx_frustum_point* d_points, int npoints, const orbx_project_item* d_items, int nitems,
                          const int32_t* d_idx, const int32_t* d_nslots, int mcap, const float* thresholds, int nlevels, int proj_kind, int rot_kind, int sum_order,
                          orbx_projmatch_point* d_out, int32_t* d_nvalid, void* stream) {
  if (!p) return ORBX_E_INVALID;
  const std::string who = "orbx_sim3_proj_device: ";
  const char* e = call_problem(d_points, npoints, d_items, nitems, d_idx, d_nslots, mcap, rot_kind, sum_order, 0, d_out, d_nvalid);
  if (!e) e = proj_problem(proj_kind);
  if (!e) e = thresholds_problem(thresholds, nlevels);
  if (e) return fail(p, ORBX_E_INVALID, who + e);
  if (proj_kind == ORBX_SIM3_PROJ_INVZ)
    return emit_device<kProjKfs>(p, who, d_points, npoints, d_items, nitems, d_idx, d_nslots, mcap, thresholds, nullptr, nlevels, rot_kind, sum_order,
                                 0, d_out, d_nvalid, stream);
  return emit_device<kProj>(p, who, d_points, npoints, d_items, nitems, d_idx, d_nslots, mcap, thresholds, nullptr, nlevels, rot_kind, sum_order, 0,
                            d_out, d_nvalid, stream);
}

int orbx_sim3_proj(orbx_sim3* p, const orbx_frustum_point* points, int npoints, const orbx_project_item* items, int nitems, const int32_t* idx,
                   const int32_t* nslots, int mcap, const float* thresholds, int nlevels, int proj_kind, int rot_kind, int sum_order,
                   orbx_projmatch_point* out, int32_t* nvalid) {
  if (!p) return ORBX_E_INVALID;
  const std::string who = "orbx_sim3_proj: ";
  const char* e = call_problem(points, npoints, items, nitems, idx, nslots, mcap, rot_kind, sum_order, 0, out, nvalid);
  if (!e) e = proj_problem(proj_kind);
  if (!e) e = thresholds_problem(thresholds, nlevels);
  if (e) return fail(p, ORBX_E_INVALID, who + e);
  if (proj_kind == ORBX_SIM3_PROJ_INVZ)
    return emit_host<kProjKfs>(p, who, points, npoints, items, nitems, idx, nslots, mcap, thresholds, nullptr, nlevels, rot_kind, sum_order, 0, out,
                               nvalid);
  return emit_host<kProj>(p, who, points, npoints, items, nitems, idx, nslots, mcap, thresholds, nullptr, nlevels, rot_kind, sum_order, 0, out, nvalid);
}

int orbx_sim3_proj_reference(const orbx_frustum_point* points, int npoints, const orbx_project_item* items, int nitems, const int32_t* idx,
                             const int32_t* nslots, int mcap, float log_scale_factor, int nlevels, int log_kind, int proj_kind, int rot_kind,
                             int sum_order, orbx_projmatch_point* out, int32_t* nvalid) {
  const char* e = call_problem(points, npoints, items, nitems, idx, nslots, mcap, rot_kind, sum_order, 0, out, nvalid);
  if (!e) e = proj_problem(proj_kind);
  if (!e) e = log_problem(log_scale_factor, nlevels, log_kind);
  if (e) return create_fail(ORBX_E_INVALID, "orbx_sim3_proj_reference", e);
  const HostLevel level = {log_scale_factor, nlevels, log_kind, nullptr};
  if (proj_kind == ORBX_SIM3_PROJ_INVZ) twin<kProjKfs>(points, npoints, items, nitems, idx, nslots, mcap, level, rot_kind, sum_order, 0, out, nvalid);
  else twin<kProj>(points, npoints, items, nitems, idx, nslots, mcap, level, rot_kind, sum_order, 0, out, nvalid);
  return ORBX_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------ fuse
int orbx_sim3_fuse_device(orbx_sim3* p, const orbx_frustum_point* d_points, int npoints, const orbx_project_item* d_items, int nitems,
                          const int32_t* d_idx, const int32_t* d_nslots, int mcap, const float* thresholds, const float* scale_factors, int nlevels,
                          int rot_kind, int sum_order, orbx_fuse_query* d_out, int32_t* d_nvalid, void* stream) {
  if (!p) return ORBX_E_INVALID;
  const std::string who = "orbx_sim3_fuse_device: ";
  const char* e = call_problem(d_points, npoints, d_items, nitems, d_idx, d_nslots, mcap, rot_kind, sum_order, 0, d_out, d_nvalid);
  if (!e) e = thresholds_problem(thresholds, nlevels);
  if (!e && !scale_factors) e = "null scale_factors";
  if (e) return fail(p, ORBX_E_INVALID, who + e);
  return emit_device<kFuse>(p, who, d_points, npoints, d_items, nitems, d_idx, d_nslots, mcap, thresholds, scale_factors, nlevels, rot_kind, sum_order,
                            0, d_out, d_nvalid, stream);
}

int orbx_sim3_fuse(orbx_sim3* p, const orbx_frustum_point* points, int npoints, const orbx_project_item* items, int nitems, const int32_t* idx,
                   const int32_t* nslots, int mcap, const float* thresholds, const float* scale_factors, int nlevels, int rot_kind, int sum_order,
                   orbx_fuse_query* out, int32_t* nvalid) {
  if (!p) return ORBX_E_INVALID;
  const std::string who = "orbx_sim3_fuse: ";
  const char* e = call_problem(points, npoints, items, nitems, idx, nslots, mcap, rot_kind, sum_order, 0, out, nvalid);
  if (!e) e = thresholds_problem(thresholds, nlevels);
  if (!e && !scale_factors) e = "null scale_factors";
  if (e) return fail(p, ORBX_E_INVALID, who + e);
  return emit_host<kFuse>(p, who, points, npoints, items, nitems, idx, nslots, mcap, thresholds, scale_factors, nlevels, rot_kind, sum_order, 0, out,
                          nvalid);
}

int orbx_sim3_fuse_reference(const orbx_frustum_point* points, int npoints, const orbx_project_item* items, int nitems, const int32_t* idx,
                             const int32_t* nslots, int mcap, float log_scale_factor, const float* scale_factors, int nlevels, int log_kind,
                             int rot_kind, int sum_order, orbx_fuse_query* out, int32_t* nvalid) {
  const char* e = call_problem(points, npoints, items, nitems, idx, nslots, mcap, rot_kind, sum_order, 0, out, nvalid);
  if (!e) e = log_problem(log_scale_factor, nlevels, log_kind);
  if (!e && !scale_factors) e = "null scale_factors";
  if (e) return create_fail(ORBX_E_INVALID, "orbx_sim3_fuse_reference", e);
  twin<kFuse>(points, npoints, items, nitems, idx, nslots, mcap, HostLevel{log_scale_factor, nlevels, log_kind, scale_factors}, rot_kind,
                   sum_order, 0, out, nvalid);
  return ORBX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------- search
int orbx_sim3_search_device(orbx_sim3* p, const orbx_frustum_point* d_points, int npoints, const orbx_sim3_item* d_items, int nitems,
                            const int32_t* d_idx, const int32_t* d_nslots, int mcap, const float* thresholds, const float* scale_factors,
                            int nlevels, int rot_kind, int sum_order, int sim_kind, orbx_fuse_query* d_out, int32_t* d_nvalid, void* stream) {
  if (!p) return ORBX_E_INVALID;
  const std::string who = "orbx_sim3_search_device: ";
  const char* e = call_problem(d_points, npoints, d_items, nitems, d_idx, d_nslots, mcap, rot_kind, sum_order, sim_kind, d_out, d_nvalid);
  if (!e) e = thresholds_problem(thresholds, nlevels);
  if (!e && !scale_factors) e = "null scale_factors";
  if (e) return fail(p, ORBX_E_INVALID, who + e);
  return emit_device<kSearch>(p, who, d_points, npoints, d_items, nitems, d_idx, d_nslots, mcap, thresholds, scale_factors, nlevels, rot_kind,
                              sum_order, sim_kind, d_out, d_nvalid, stream);
}

int orbx_sim3_search(orbx_sim3* p, const orbx_frustum_point* points, int npoints, const orbx_sim3_item* items, int nitems, const int32_t* idx,
                     const int32_t* nslots, int mcap, const float* thresholds, const float* scale_factors, int nlevels, int rot_kind, int sum_order,
                     int sim_kind, orbx_fuse_query* out, int32_t* nvalid) {
  if (!p) return ORBX_E_INVALID;
  const std::string who = "orbx_sim3_search: ";
  const char* e = call_problem(points, npoints, items, nitems, idx, nslots, mcap, rot_kind, sum_order, sim_kind, out, nvalid);
  if (!e) e = thresholds_problem(thresholds, nlevels);
  if (!e && !scale_factors) e = "null scale_factors";
  if (e) return fail(p, ORBX_E_INVALID, who + e);
  return emit_host<kSearch>(p, who, points, npoints, items, nitems, idx, nslots, mcap, thresholds, scale_factors, nlevels, rot_kind, sum_order,
                            sim_kind, out, nvalid);
}

int orbx_sim3_search_reference(const orbx_frustum_point* points, int npoints, const orbx_sim3_item* items, int nitems, const int32_t* idx,
                               const int32_t* nslots, int mcap, float log_scale_factor, const float* scale_factors, int nlevels, int log_kind,
                               int rot_kind, int sum_order, int sim_kind, orbx_fuse_query* out, int32_t* nvalid) {
  const char* e = call_problem(points, npoints, items, nitems, idx, nslots, mcap, rot_kind, sum_order, sim_kind, out, nvalid);
  if (!e) e = log_problem(log_scale_factor, nlevels, log_kind);
  if (!e && !scale_factors) e = "null scale_factors";
  if (e) return create_fail(ORBX_E_INVALID, "orbx_sim3_search_reference", e);
  twin<kSearch>(points, npoints, items, nitems, idx, nslots, mcap, HostLevel{log_scale_factor, nlevels, log_kind, scale_factors}, rot_kind,
                     sum_order, sim_kind, out, nvalid);
  return ORBX_OK;
}

// ----------------------------------------------------------------------------------------------------------------------------------- agree
int orbx_sim3_agree_device(orbx_sim3* p, const int32_t* d_best_idx12, const int32_t* d_best_dist12, const int32_t* d_nfound12,
                           const int32_t* d_best_idx21, const int32_t* d_best_dist21, const int32_t* d_nfound21, const int32_t* d_n1,
                           const int32_t* d_n2, int npairs, int qcap, int th_high, int32_t* d_match12, int32_t* d_nfound, void* stream) {
  if (!p) return ORBX_E_INVALID;
  const std::string who = "orbx_sim3_agree_device: ";
  if (const char* e = agree_problem(d_best_idx12, d_best_dist12, d_nfound12, d_best_idx21, d_best_dist21, d_nfound21, d_n1, d_n2, npairs, qcap,
                                    d_match12, d_nfound))
    return fail(p, ORBX_E_INVALID, who + e);
  int chunks;
  if (const char* e = grid_problem(0, nullptr, npairs, qcap, &chunks)) return fail(p, ORBX_E_INVALID, who + e);
  int rc = same_device(p, who.c_str(), {d_best_idx12, d_best_dist12, d_nfound12, d_best_idx21, d_best_dist21, d_nfound21, d_n1, d_n2, d_match12, d_nfound},
                       "the handle");
  if (rc != ORBX_OK) return rc;
  const AgreeArgs g = {d_best_idx12, d_best_dist12, d_nfound12, d_best_idx21, d_best_dist21, d_nfound21, d_n1, d_n2, d_match12, d_nfound,
                       npairs, qcap, chunks, th_high};
  ORBX_SIDE_HIP(p, hipSetDevice(p->device));
  hipStream_t st = stream ? (hipStream_t)stream : p->st;
  if ((rc = wait_previous(p, st)) != ORBX_OK) return rc;
  hipLaunchKernelGGL(k_sim3_agree_check, dim3((unsigned)((npairs + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, g);
  hipLaunchKernelGGL(k_sim3_agree, dim3((unsigned)(npairs * chunks)), dim3(kThreads), 0, st, g);
  return record_call(p, st);
}

int orbx_sim3_agree(orbx_sim3* p, const int32_t* best_idx12, const int32_t* best_dist12, const int32_t* nfound12, const int32_t* best_idx21,
                    const int32_t* best_dist21, const int32_t* nfound21, const int32_t* n1, const int32_t* n2, int npairs, int qcap, int th_high,
                    int32_t* match12, int32_t* nfound) {
  if (!p) return ORBX_E_INVALID;
  const std::string who = "orbx_sim3_agree: ";
  if (const char* e = agree_problem(best_idx12, best_dist12, nfound12, best_idx21, best_dist21, nfound21, n1, n2, npairs, qcap, match12, nfound))
    return fail(p, ORBX_E_INVALID, who + e);
  Stager io;
  const size_t block = (size_t)npairs * qcap * 4, vec = (size_t)npairs * 4;
  const size_t o_i12 = io.in(best_idx12, block), o_d12 = io.in(best_dist12, block), o_f12 = io.in(nfound12, vec);
  const size_t o_i21 = io.in(best_idx21, block), o_d21 = io.in(best_dist21, block), o_f21 = io.in(nfound21, vec);
  const size_t o_n1 = io.in(n1, vec), o_n2 = io.in(n2, vec);
  const size_t o_match = io.out(match12, block), o_nfound = io.out(nfound, vec);
  int rc = upload(p, io);
  if (rc != ORBX_OK) return rc;
  const int32_t* const d = (const int32_t*)p->io.p;
  int32_t* const w = (int32_t*)p->io.p;
  rc = orbx_sim3_agree_device(p, d + o_i12 / 4, d + o_d12 / 4, d + o_f12 / 4, d + o_i21 / 4, d + o_d21 / 4, d + o_f21 / 4, d + o_n1 / 4, d + o_n2 / 4,
                              npairs, qcap, th_high, w + o_match / 4, w + o_nfound / 4, p->st);
  if (rc != ORBX_OK) return rc;
  return download(p, io);
}

int orbx_sim3_agree_reference(const int32_t* best_idx12, const int32_t* best_dist12, const int32_t* nfound12, const int32_t* best_idx21,
                              const int32_t* best_dist21, const int32_t* nfound21, const int32_t* n1, const int32_t* n2, int npairs, int qcap,
                              int th_high, int32_t* match12, int32_t* nfound) {
  if (const char* e = agree_problem(best_idx12, best_dist12, nfound12, best_idx21, best_dist21, nfound21, n1, n2, npairs, qcap, match12, nfound))
    return create_fail(ORBX_E_INVALID, "orbx_sim3_agree_reference", e);
  for (int p = 0; p < npairs; p++) {
    const bool bad = pair_is_bad(nfound12[p], nfound21[p], n1[p], n2[p], qcap);
    const size_t row = (size_t)p * qcap;
    int count = 0;
    for (int i1 = 0; i1 < qcap; i1++) {
      int m = -1;
      if (!bad && i1 < n1[p]) m = agree_one(i1, best_idx12[row + i1], best_dist12[row + i1], n2[p], th_high, Match2{best_idx21 + row, best_dist21 + row, th_high});
      match12[row + i1] = m;
      count += m >= 0;
    }
    nfound[p] = bad ? -1 : count;
  }
  return ORBX_OK;
}

}  // extern "C"
