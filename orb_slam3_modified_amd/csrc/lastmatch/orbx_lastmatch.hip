// The batched frame-to-last-frame matcher (include/orbx_lastmatch.h): ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame&
// LastFrame, th, bMono) (src/ORBmatcher.cc:1676-1885, Nleft == -1) for B (current frame, last frame's points) items on the keypoints and
// descriptors a batch extraction left in HBM and the points' descriptors in the pool ComputeDistinctiveDescriptors fills.
//
// k_last_match<LDS>: one workgroup of 8 waves per item (a grid of at most kMaxBlocks workgroups walks the items).  The frame grid, the
// window walk, the offsets' scan, the chunk cut, the chain's step (the scan over the open candidates, the bind), the last writer, the
// rotation filter and the two paths' layout are csrc/side/orbx_window_device.h's; this file holds what is this matcher's own:
//   check                the item's frame, count, nlast, direction and th and every valid point's octave and pool row, before any of them
//                        addresses memory.
//   phase A              the window GetFeaturesInArea(u, v, radius, the direction's level range) with the stereo gate; a candidate is one
//                        word: index (15 bits), Hamming distance (9).  The kp_obs test is the chain's.  (Only a best is kept, so entries
//                        above 100 could be left out of the lists; they are not: leaving them out would need the distances in the counting
//                        walk too, and the chain passes over them in the same trip.)
//   phase B, wave 0      the walk over the chunk's points in index order; a step is the core's on the smallest key of the candidates whose
//                        keypoint is not hidden (a bit per keypoint in LDS, from the kp_obs row, set on every acceptance with obs > 0): the
//                        first in walk order among equal distances, accepted at a distance of at most 100 (:1770).  The accept test is
//                        wave-uniform.  No descriptor and no keypoint is read here.  A and B repeat per chunk: the distances do not depend
//                        on the chain, so where the chunks are cut changes nothing.
//   phase C, all waves   the core's last writer.
//   phase D, all waves   under check_orientation, the core's rotation filter: every entry of a bin outside the three maxima writes
//                        kp_match = -2, kp_obs = -1: entries of one keypoint write the same values, so nothing depends on the order.
// The hidden bits are 4 KiB of static LDS on both paths.
// The float expressions are compiled with -ffp-contract=off: every operation is rounded by itself, as the specification states them.
#include <hip/hip_runtime.h>

#include <string>

#include "../side/orbx_handle.h"
#include "../side/orbx_pair_device.h"
#include "../side/orbx_window_device.h"
#include "../side/orbx_window_host.h"
#include "../../../include/orbx_lastmatch.h"

struct orbx_lastmatch : orbx::side::win::WindowHandle {};   // lds_limit: ORBX_LASTMATCH_LDS at create

namespace {

using namespace orbx::side;
using namespace orbx::side::dev;
using namespace orbx::side::win;

static_assert(ORBX_LASTMATCH_MAX_CAPACITY == kMaxCap && ORBX_LASTMATCH_MAX_LEVELS == kMaxLevels, "the window core's limits");

struct Args {
  const uint8_t* kps; const uint8_t* desc; const int32_t* counts; const float* uright; const float* bounds;
  const orbx_lastmatch_item* items; const orbx_lastmatch_point* pts; const int32_t* nlast; const uint8_t* pdesc;
  int32_t* kp_obs; int32_t* kp_match; int32_t* nmatches;
  uint8_t* scratch; size_t scratch_stride;
  int nframes, cap, nitems, mcap, npoints, nlevels, p2, room, check_ori;
  float sf[kMaxLevels];
};

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
  __shared__ int s_bad;
  __shared__ int32_t s_hidden[kMaxCap / 32];   // bit i: keypoint i holds a map point with Observations() > 0
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
    if (tid == 0) s_bad = 0;
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
    const uint8_t* const desc = LDS ? base + L.desc : g.desc + of * 32;
    const Grid G = frame_grid(g.bounds + 4 * f);

    // ---- phase A: the frame's grid, the hidden bits in the same trip over the keypoints
    if (LDS) stage_dma<kThreads>(base + L.desc, g.desc + of * 32, n * 2);
    for (int w = tid; w < kMaxCap / 32; w += kThreads) s_hidden[w] = 0;
    for (int q = tid; q < nlast; q += kThreads) res[q] = -1;
    build_grid<kThreads>(G, kp, g.uright ? g.uright + of : nullptr, n, A, [&](int i) { if (oobs[i] > 0) set_bit(s_hidden, i); });

    // ---- phase A: every point's candidate count, then the offsets
    for (int q = tid; q <= nlast; q += kThreads) {
      int c = 0;
      if (q < nlast) {
        const Pt t = load_point(pts + q, s_sf, th, mbf, direction);
        if (t.live)
          walk<false>(G, t.x, t.y, t.radius, t.lo, t.hi, A, [&](const Rec& r, int) {
            if (r.ur > 0.0f && fabsf(t.xr - r.ur) > t.radius) return;   // the stereo gate, src/ORBmatcher.cc:1751-1757
            c++;
          });
      }
      offs[q] = c;
    }
    scan_offsets<kThreads>(offs, nlast + 1);
    if (LDS) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the LDS-DMA loads have landed
    __syncthreads();

    // ---- chunks of points whose candidates fit the room: lists with distances (all waves), then the chain (wave 0)
    int nm = 0;                            // wave 0's count of acceptances
    for (int q0 = 0; q0 < nlast;) {
      const int e0 = offs[q0], q1 = chunk_end(offs, q0, nlast, g.room);
      const int tot = min(offs[q1] - e0, g.room);
      for (int q = q0 + tid; q < q1; q += kThreads) {
        int k = offs[q] - e0;
        const int kend = offs[q + 1] - e0;
        if (kend > k) {
          const Pt t = load_point(pts + q, s_sf, th, mbf, direction);
          const D8 qd = load_desc(g.pdesc + (size_t)t.point * 32);   // the pool row is below npoints: the check
          walk<false>(G, t.x, t.y, t.radius, t.lo, t.hi, A, [&](const Rec& r, int i) {
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
            const int m1 = open_top(cand, b0, cnt, 0, s_hidden, lane);
            if (m1 == kNone || (m1 >> 15) > kThHigh) continue;   // :1770
            const int obs = __builtin_amdgcn_readlane(l_obs, i);
            if (lane == 0) bind<false>(s_hidden, res + c0 + i, (int)(cand[b0 + (m1 & 0x7FFF)] & 0x7FFFu), obs);   // the slot was open: obs <= 0 leaves its bit clear
            nm++;
            publish();
          }
        }
      }
#endif
      __syncthreads();
      q0 = q1;
    }

    last_writer<kThreads, 1>(res, nlast, n, omatch, oobs, [&](int q) { return pts[q].obs; });   // ---- phase C
    int removed = 0;
#ifndef ORBX_LASTMATCH_NO_HIST             // (a timing build without phase D: tools/lastmatch_times.py)
    // ---- phase D: the rotation histogram (:1775-1792), its three maxima and the removal (:1862-1882)
    if (g.check_ori)                       // uniform over the grid; its first barrier: phase C's reads of kp_match and writes of kp_obs are done
      removed = rotation_filter<kThreads, 1>(res, nlast, n, [&](int q) { return pts[q].angle; }, [&](int i) { return kp_field<float>(kp, i, kAngle); },
                                             [&](int i) { omatch[i] = -2; oobs[i] = -1; });
#endif
    if (tid == 0) g.nmatches[b] = nm - removed;
  }
}

// what both forms check before anything is copied or launched
int check(orbx_lastmatch* m, const char* who, const orbx_lastmatch_side* side, const void* items, int nitems, const void* points, const void* nlast,
          int mcap, const void* pdesc, int npoints, const float* sf, int nlevels, const void* kp_obs, const void* kp_match, const void* nmatches) {
  return check_call(m, who, side, items && points && nlast && pdesc, "items, points, nlast or pdesc", kp_obs && kp_match && nmatches,
                    "kp_obs, kp_match or nmatches", nitems, mcap, npoints, sf, nlevels);
}

}  // namespace

extern "C" {

int orbx_lastmatch_create(orbx_lastmatch** out, int device) {
  return create_handle(out, device, "orbx_lastmatch_create", orbx_lastmatch_destroy,
                       [](orbx_lastmatch* m) { return open_window(m, "ORBX_LASTMATCH_LDS", (const void*)k_last_match<true>); });
}

void orbx_lastmatch_destroy(orbx_lastmatch* m) { destroy_handle(m); }

const char* orbx_lastmatch_last_error(const orbx_lastmatch* m) { return last_error(m); }

int orbx_lastmatch_search_device(orbx_lastmatch* m, const orbx_lastmatch_side* side, const orbx_lastmatch_item* d_items, int nitems,
                                 const orbx_lastmatch_point* d_points, const int32_t* d_nlast, int mcap, const uint8_t* d_pdesc, int npoints,
                                 const float* scale_factors, int nlevels, int check_orientation, int32_t* d_kp_obs, int32_t* d_kp_match,
                                 int32_t* d_nmatches, void* stream) {
  if (!m) return ORBX_E_INVALID;
  const char* who = "orbx_lastmatch_search_device: ";
  int rc = check(m, who, side, d_items, nitems, d_points, d_nlast, mcap, d_pdesc, npoints, scale_factors, nlevels, d_kp_obs, d_kp_match, d_nmatches);
  if (rc != ORBX_OK) return rc;
  if (((uintptr_t)side->d_desc | (uintptr_t)d_points | (uintptr_t)d_pdesc) & 15)
    return fail(m, ORBX_E_INVALID, std::string(who) + "d_desc, d_points and d_pdesc must be 16-byte aligned");
  rc = same_device(m, who, {side->d_kps, side->d_desc, side->d_counts, side->d_uright, side->d_bounds, d_items, d_points, d_nlast, d_pdesc,
                            d_kp_obs, d_kp_match, d_nmatches}, "the handle");
  if (rc != ORBX_OK) return rc;
  ORBX_SIDE_HIP(m, hipSetDevice(m->device));
  const int cap = side->capacity;
  int p2;
  Paths path;
  if ((rc = plan(m, cap, mcap, nitems, &p2, &path)) != ORBX_OK) return rc;
  Args g;
  g.kps = (const uint8_t*)side->d_kps; g.desc = side->d_desc; g.counts = side->d_counts; g.uright = side->d_uright; g.bounds = side->d_bounds;
  g.items = d_items; g.pts = d_points; g.nlast = d_nlast; g.pdesc = d_pdesc;
  g.kp_obs = d_kp_obs; g.kp_match = d_kp_match; g.nmatches = d_nmatches;
  g.nframes = side->nframes; g.cap = cap; g.nitems = nitems; g.mcap = mcap; g.npoints = npoints; g.nlevels = nlevels; g.p2 = p2;
  g.check_ori = check_orientation != 0;
  fill_levels(g.sf, scale_factors, nlevels);
  return launch(m, path, g, k_last_match<true>, k_last_match<false>, stream);
}

int orbx_lastmatch_search(orbx_lastmatch* m, const orbx_lastmatch_side* side, const orbx_lastmatch_item* items, int nitems,
                          const orbx_lastmatch_point* points, const int32_t* nlast, int mcap, const uint8_t* pdesc, int npoints,
                          const float* scale_factors, int nlevels, int check_orientation, int32_t* kp_obs, int32_t* kp_match,
                          int32_t* nmatches) {
  if (!m) return ORBX_E_INVALID;
  const char* who = "orbx_lastmatch_search: ";
  int rc = check(m, who, side, items, nitems, points, nlast, mcap, pdesc, npoints, scale_factors, nlevels, kp_obs, kp_match, nmatches);
  if (rc != ORBX_OK) return rc;
  Stager io;
  const size_t rows = (size_t)nitems * side->capacity;
  const StagedSide ss = stage_side(io, side, &orbx_lastmatch_side::d_uright);
  const size_t o_items = io.in(items, (size_t)nitems * sizeof(orbx_lastmatch_item));
  const size_t o_pts = io.in(points, (size_t)nitems * mcap * sizeof(orbx_lastmatch_point));
  const size_t o_nlast = io.in(nlast, (size_t)nitems * 4), o_pdesc = io.in(pdesc, (size_t)npoints * 32);
  const size_t o_obs = io.out(kp_obs, rows * 4, true), o_match = io.out(kp_match, rows * 4), o_nm = io.out(nmatches, (size_t)nitems * 4);
  if ((rc = upload(m, io)) != ORBX_OK) return rc;
  uint8_t* const d = m->io.p;
  const orbx_lastmatch_side ds = device_side(d, ss, side, &orbx_lastmatch_side::d_uright);
  rc = orbx_lastmatch_search_device(m, &ds, (const orbx_lastmatch_item*)(d + o_items), nitems, (const orbx_lastmatch_point*)(d + o_pts),
                                    (const int32_t*)(d + o_nlast), mcap, d + o_pdesc, npoints, scale_factors, nlevels, check_orientation,
                                    (int32_t*)(d + o_obs), (int32_t*)(d + o_match), (int32_t*)(d + o_nm), m->st);
  if (rc != ORBX_OK) return rc;
  return download(m, io);
}

}  // extern "C"
