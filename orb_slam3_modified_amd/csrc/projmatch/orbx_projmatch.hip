// The batched relocalization and Sim3 matchers (include/orbx_projmatch.h): ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF,
// sAlreadyFound, th, ORBdist) (src/ORBmatcher.cc:1889-2010, kind 0) and SearchByProjection(KeyFrame*, Sim3f& Scw, vpPoints[, vpPointsKFs],
// vpMatched[, vpMatchedKF], th, ratioHamming) (:427-532, :534-646, kind 1) for B (frame, projected points) items on the keypoints and
// descriptors a batch extraction left in HBM and the points' descriptors in the pool ComputeDistinctiveDescriptors fills.
//
// k_proj_match<LDS>: one workgroup of 8 waves per item (a grid of at most kMaxBlocks workgroups walks the items).  The frame grid, the
// window walk, the offsets' scan, the chunk cut, the chain's step (the scan over the open candidates, the bind), the rotation filter and
// the two paths' layout are csrc/side/orbx_window_device.h's; this file holds what is this matcher's own:
//   check                the item's frame, count, npts, kind and th and every valid point's level and pool row, before any of them
//                        addresses memory.
//   phase A              the window GetFeaturesInArea(u, v, radius, level - 1, level + 1 - kind), no stereo gate (the records' right
//                        coordinate is -1); for kind 1 the reference applies the range in its walk over an unfiltered list, :509 / :622: the
//                        same keypoints in the same order.  A candidate is one word: index (15 bits), Hamming distance (9).  The taken test
//                        is the chain's.  (Only a best is kept, so entries above the item's max_dist could be left out of the lists; they
//                        are not: see DESIGN.md section 21.)
//   phase B, wave 0      the walk over the chunk's points in index order; a step is the core's on the smallest key of the candidates whose
//                        keypoint is not taken (a bit per keypoint in LDS, from the kp_taken row, set on every acceptance; :504, :1952):
//                        the first in walk order among equal distances.  The accept test, a float compare against the item's max_dist, is
//                        wave-uniform; the binding lane writes kp_match too: there is no phase C.  No descriptor and no keypoint is read
//                        here.  A and B repeat per chunk: the distances do not depend on the chain, so where the chunks are cut changes
//                        nothing.
//   phase D, all waves   kind 0 under check_orientation, the core's rotation filter: every entry of a bin outside the three maxima writes
//                        kp_match = -2.  A keypoint is bound at most once per row, so every entry is a keypoint of its own.
// The taken bits are 4 KiB of static LDS on both paths.
// The float expressions are compiled with -ffp-contract=off: every operation is rounded by itself, as the specification states them.
#include <hip/hip_runtime.h>

#include <string>

#include "../side/orbx_handle.h"
#include "../side/orbx_pair_device.h"
#include "../side/orbx_window_device.h"
#include "../side/orbx_window_host.h"
#include "../../../include/orbx_projmatch.h"

struct orbx_projmatch : orbx::side::win::WindowHandle {};   // lds_limit: ORBX_PROJMATCH_LDS at create

namespace {

using namespace orbx::side;
using namespace orbx::side::dev;
using namespace orbx::side::win;

static_assert(ORBX_PROJMATCH_MAX_CAPACITY == kMaxCap && ORBX_PROJMATCH_MAX_LEVELS == kMaxLevels, "the window core's limits");
static_assert(sizeof(orbx_projmatch_item) == 16 && sizeof(orbx_projmatch_point) == 32, "the ABI's records");

struct Args {
  const uint8_t* kps; const uint8_t* desc; const int32_t* counts; const float* bounds;
  const orbx_projmatch_item* items; const orbx_projmatch_point* pts; const int32_t* npts; const uint8_t* pdesc;
  const uint8_t* kp_taken; int32_t* kp_match; int32_t* nmatches;
  uint8_t* scratch; size_t scratch_stride;
  int nframes, cap, nitems, mcap, npoints, nlevels, p2, room, check_ori;
  float sf[kMaxLevels];
};

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
  __shared__ int s_bad;
  __shared__ int32_t s_taken[kMaxCap / 32];    // bit i: keypoint i holds a map point
  __shared__ float s_sf[kMaxLevels];
  const int tid = threadIdx.x, lane = tid & 63;
  const int cap = g.cap, mcap = g.mcap;
  const Lay L = layout(cap, mcap, g.p2, LDS);
  uint8_t* const base = LDS ? smem : g.scratch + (size_t)blockIdx.x * g.scratch_stride;
  const Arrays A = arrays(base, L, L.grid);
  int32_t *const offs = A.offs, *const res = A.res;
  uint32_t* const cand = A.cand;
  load_levels(s_sf, g.sf);

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
    if (tid == 0) s_bad = 0;
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
    const Grid G = frame_grid(g.bounds + 4 * f);

    // ---- phase A: the frame's grid, the taken bits in the same trip over the keypoints
    if (LDS) stage_dma<kThreads>(base + L.desc, g.desc + of * 32, n * 2);
    for (int w = tid; w < kMaxCap / 32; w += kThreads) s_taken[w] = 0;
    for (int q = tid; q < npts; q += kThreads) res[q] = -1;
    build_grid<kThreads>(G, kp, nullptr, n, A, [&](int i) { if (taken && taken[i]) set_bit(s_taken, i); });

    // ---- phase A: every point's candidate count, then the offsets
    for (int q = tid; q <= npts; q += kThreads) {
      int c = 0;
      if (q < npts) {
        const Pt t = load_point(pts + q, s_sf, th);
        if (t.live) walk<true>(G, t.x, t.y, t.radius, t.level - 1, t.level + up, A, [&](const Rec&, int) { c++; });
      }
      offs[q] = c;
    }
    scan_offsets<kThreads>(offs, npts + 1);
    if (LDS) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the LDS-DMA loads have landed
    __syncthreads();

    // ---- chunks of points whose candidates fit the room: lists with distances (all waves), then the chain (wave 0)
    int nm = 0;                            // wave 0's count of acceptances
    for (int q0 = 0; q0 < npts;) {
      const int e0 = offs[q0], q1 = chunk_end(offs, q0, npts, g.room);
      const int tot = min(offs[q1] - e0, g.room);
      for (int q = q0 + tid; q < q1; q += kThreads) {
        int k = offs[q] - e0;
        const int kend = offs[q + 1] - e0;
        if (kend > k) {
          const Pt t = load_point(pts + q, s_sf, th);
          const D8 qd = load_desc(g.pdesc + (size_t)t.point * 32);   // the pool row is below npoints: the check
          walk<true>(G, t.x, t.y, t.radius, t.level - 1, t.level + up, A, [&](const Rec&, int i) {
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
            const int m1 = open_top(cand, b0, cnt, 0, s_taken, lane);
            if (m1 == kNone || !((float)(m1 >> 15) <= max_dist)) continue;   // :523, :636, :1966; a NaN limit accepts nothing
            if (lane == 0) {
              const int idx = (int)(cand[b0 + (m1 & 0x7FFF)] & 0x7FFFu);     // below n: a candidate is a keypoint of the grid
              omatch[idx] = c0 + i;
              bind<false>(s_taken, res + c0 + i, idx, 1);
            }
            nm++;
            publish();
          }
        }
      }
#endif
      __syncthreads();
      q0 = q1;
    }

    int removed = 0;
#ifndef ORBX_PROJMATCH_NO_HIST             // (a timing build without phase D: tools/projmatch_times.py)
    // ---- phase D: the rotation histogram (:1971-1981), its three maxima and the removal (:1988-2007); the Sim3 overloads have none
    if (g.check_ori && kind == 0)          // uniform over the workgroup; -2 after the chain's store to the same word: barriers lie between them
      removed = rotation_filter<kThreads, 1>(res, npts, n, [&](int q) { return pts[q].angle; }, [&](int i) { return kp_field<float>(kp, i, kAngle); },
                                             [&](int i) { omatch[i] = -2; });
#endif
    if (tid == 0) g.nmatches[b] = nm - removed;
  }
}

// what both forms check before anything is copied or launched
int check(orbx_projmatch* m, const char* who, const orbx_projmatch_side* side, const void* items, int nitems, const void* points, const void* npts,
          int mcap, const void* pdesc, int npoints, const float* sf, int nlevels, const void* kp_match, const void* nmatches) {
  return check_call(m, who, side, items && points && npts && pdesc, "items, points, npts or pdesc", kp_match && nmatches, "kp_match or nmatches",
                    nitems, mcap, npoints, sf, nlevels);
}

}  // namespace

extern "C" {

int orbx_projmatch_create(orbx_projmatch** out, int device) {
  return create_handle(out, device, "orbx_projmatch_create", orbx_projmatch_destroy,
                       [](orbx_projmatch* m) { return open_window(m, "ORBX_PROJMATCH_LDS", (const void*)k_proj_match<true>); });
}

void orbx_projmatch_destroy(orbx_projmatch* m) { destroy_handle(m); }

const char* orbx_projmatch_last_error(const orbx_projmatch* m) { return last_error(m); }

int orbx_projmatch_search_device(orbx_projmatch* m, const orbx_projmatch_side* side, const orbx_projmatch_item* d_items, int nitems,
                                 const orbx_projmatch_point* d_points, const int32_t* d_npts, int mcap, const uint8_t* d_pdesc, int npoints,
                                 const float* scale_factors, int nlevels, int check_orientation, const uint8_t* d_kp_taken,
                                 int32_t* d_kp_match, int32_t* d_nmatches, void* stream) {
  if (!m) return ORBX_E_INVALID;
  const char* who = "orbx_projmatch_search_device: ";
  int rc = check(m, who, side, d_items, nitems, d_points, d_npts, mcap, d_pdesc, npoints, scale_factors, nlevels, d_kp_match, d_nmatches);
  if (rc != ORBX_OK) return rc;
  if (((uintptr_t)side->d_desc | (uintptr_t)d_points | (uintptr_t)d_pdesc) & 15)
    return fail(m, ORBX_E_INVALID, std::string(who) + "d_desc, d_points and d_pdesc must be 16-byte aligned");
  rc = same_device(m, who, {side->d_kps, side->d_desc, side->d_counts, side->d_bounds, d_items, d_points, d_npts, d_pdesc, d_kp_taken,
                            d_kp_match, d_nmatches}, "the handle");
  if (rc != ORBX_OK) return rc;
  ORBX_SIDE_HIP(m, hipSetDevice(m->device));
  const int cap = side->capacity;
  int p2;
  Paths path;
  if ((rc = plan(m, cap, mcap, nitems, &p2, &path)) != ORBX_OK) return rc;
  Args g;
  g.kps = (const uint8_t*)side->d_kps; g.desc = side->d_desc; g.counts = side->d_counts; g.bounds = side->d_bounds;
  g.items = d_items; g.pts = d_points; g.npts = d_npts; g.pdesc = d_pdesc;
  g.kp_taken = d_kp_taken; g.kp_match = d_kp_match; g.nmatches = d_nmatches;
  g.nframes = side->nframes; g.cap = cap; g.nitems = nitems; g.mcap = mcap; g.npoints = npoints; g.nlevels = nlevels; g.p2 = p2;
  g.check_ori = check_orientation != 0;
  fill_levels(g.sf, scale_factors, nlevels);
  return launch(m, path, g, k_proj_match<true>, k_proj_match<false>, stream);
}

int orbx_projmatch_search(orbx_projmatch* m, const orbx_projmatch_side* side, const orbx_projmatch_item* items, int nitems,
                          const orbx_projmatch_point* points, const int32_t* npts, int mcap, const uint8_t* pdesc, int npoints,
                          const float* scale_factors, int nlevels, int check_orientation, const uint8_t* kp_taken, int32_t* kp_match,
                          int32_t* nmatches) {
  if (!m) return ORBX_E_INVALID;
  const char* who = "orbx_projmatch_search: ";
  int rc = check(m, who, side, items, nitems, points, npts, mcap, pdesc, npoints, scale_factors, nlevels, kp_match, nmatches);
  if (rc != ORBX_OK) return rc;
  Stager io;
  const size_t rows = (size_t)nitems * side->capacity;
  const StagedSide ss = stage_side(io, side);
  const size_t o_items = io.in(items, (size_t)nitems * sizeof(orbx_projmatch_item));
  const size_t o_pts = io.in(points, (size_t)nitems * mcap * sizeof(orbx_projmatch_point));
  const size_t o_npts = io.in(npts, (size_t)nitems * 4), o_pdesc = io.in(pdesc, (size_t)npoints * 32);
  const size_t o_taken = kp_taken ? io.in(kp_taken, rows) : 0;
  const size_t o_match = io.out(kp_match, rows * 4), o_nm = io.out(nmatches, (size_t)nitems * 4);
  if ((rc = upload(m, io)) != ORBX_OK) return rc;
  uint8_t* const d = m->io.p;
  const orbx_projmatch_side ds = device_side(d, ss, side);
  rc = orbx_projmatch_search_device(m, &ds, (const orbx_projmatch_item*)(d + o_items), nitems, (const orbx_projmatch_point*)(d + o_pts),
                                    (const int32_t*)(d + o_npts), mcap, d + o_pdesc, npoints, scale_factors, nlevels, check_orientation,
                                    kp_taken ? d + o_taken : nullptr, (int32_t*)(d + o_match), (int32_t*)(d + o_nm), m->st);
  if (rc != ORBX_OK) return rc;
  return download(m, io);
}

}  // extern "C"
