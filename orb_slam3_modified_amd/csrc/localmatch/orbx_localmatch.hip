// The batched SearchLocalPoints (include/orbx_localmatch.h): ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th, ...)
// (src/ORBmatcher.cc:43-141, Nleft == -1) for B (frame, local map) items on the keypoints and descriptors a batch extraction left in HBM
// and the map points' descriptors in the pool ComputeDistinctiveDescriptors fills.
//
// k_local_match<LDS>: one workgroup of 8 waves per item (a grid of at most kMaxBlocks workgroups walks the items).  The frame grid, the
// window walk, the offsets' scan, the chunk cut and the two paths' layout are csrc/side/orbx_window_device.h's; this file holds what is
// this matcher's own:
//   check                the item's frame, count, nmp and every in-view point's level and pool row, before any of them addresses memory.
//   phase A              the window GetFeaturesInArea(x, y, radius, level - 1, level) with the stereo gate; a candidate is one word: index
//                        (15 bits), Hamming distance (9), octave (5, two's complement: -1 .. 15).  The kp_obs test is the chain's.
//   phase B, wave 0      the chain over the chunk's points in index order: lane j holds candidate j (+ 64 per trip), drops the entries whose
//                        keypoint is hidden (a bit per keypoint in LDS, from the kp_obs row, set on every acceptance with obs > 0), keeps its
//                        two smallest (distance << 15 | position) keys; two DPP min-reductions give the wave's two smallest, whose entries
//                        carry the octaves.  The accept test is wave-uniform; one lane records the point's keypoint and sets the hidden bit.
//                        No descriptor and no keypoint is read here.  A and B repeat per chunk: the distances do not depend on the chain,
//                        so where the chunks are cut changes nothing.
//   phase C, all waves   kp_match[keypoint] = the LAST accepted point that took it (an integer maximum over the points' indices: a point
//                        with obs == 0 does not hide its keypoint, a later one may rebind it), then kp_obs[keypoint] = that point's obs.
// The hidden bits are 4 KiB of static LDS on both paths.
// The float expressions are compiled with -ffp-contract=off: every operation is rounded by itself, as the specification states them.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../side/orbx_handle.h"
#include "../side/orbx_pair_device.h"
#include "../side/orbx_window_device.h"
#include "../side/orbx_window_host.h"
#include "../../../include/orbx_localmatch.h"

struct orbx_localmatch : orbx::side::win::WindowHandle {};   // lds_limit: ORBX_LOCALMATCH_LDS at create

namespace {

using namespace orbx::side;
using namespace orbx::side::dev;          // ld / st on the chain's state: written by one lane, read by the wave's other lanes in the next step
using namespace orbx::side::win;

constexpr int kThHigh = 100;
static_assert(ORBX_LOCALMATCH_MAX_CAPACITY == kMaxCap && ORBX_LOCALMATCH_MAX_LEVELS == kMaxLevels, "the window core's limits");

struct Args {
  const uint8_t* kps; const uint8_t* desc; const int32_t* counts; const float* uright; const float* bounds;
  const int32_t* frames; const orbx_localmatch_point* mp; const int32_t* nmp; const uint8_t* pdesc;
  int32_t* kp_obs; int32_t* kp_match; int32_t* nmatches;
  uint8_t* scratch; size_t scratch_stride;
  int nframes, cap, nitems, mcap, npoints, nlevels, p2, room, factor;
  float th, ratio;
  float sf[kMaxLevels];
};

// a point's window: RadiusByViewingCos (src/ORBmatcher.cc:214-220), th, the level's scale
struct Pt { float x, y, xr, radius; int level, point; bool live; };
__device__ __forceinline__ Pt load_point(const orbx_localmatch_point* p, const float* s_sf, float th, int factor) {
  const uint4* const rp = (const uint4*)p;
  const uint4 lo = rp[0], hi = rp[1];
  Pt t;
  t.x = __uint_as_float(lo.x); t.y = __uint_as_float(lo.y); t.xr = __uint_as_float(lo.z);
  const float vc = __uint_as_float(lo.w);
  t.level = (int)hi.x; t.point = (int)hi.z;
  // in view, and finite: a NaN fails every comparison (the reference leaves a non-finite projection undefined; here it has no candidate)
  t.live = hi.w != 0u && fabsf(t.x) < INFINITY && fabsf(t.y) < INFINITY && fabsf(vc) < INFINITY;
  t.radius = 0.0f;
  if (t.live) {                            // the level is one of the table's: the check
    float r = ((double)vc > 0.998) ? 2.5f : 4.0f;
    if (factor) r *= th;
    t.radius = r * s_sf[t.level];
  }
  return t;
}

template <bool LDS>
__global__ __launch_bounds__(kThreads) void k_local_match(Args g) {
  extern __shared__ __align__(16) uint8_t smem[];
  __shared__ int s_bad;
  __shared__ int32_t s_hidden[kMaxCap / 32];   // bit i: keypoint i holds a map point with Observations() > 0
  __shared__ float s_sf[kMaxLevels];
  const int tid = threadIdx.x, lane = tid & 63;
  const int cap = g.cap, mcap = g.mcap;
  const Lay L = layout(cap, mcap, g.p2, LDS);
  uint8_t* const base = LDS ? smem : g.scratch + (size_t)blockIdx.x * g.scratch_stride;
  const Arrays A = arrays(base, L);
  int32_t *const offs = A.offs, *const res = A.res;
  uint32_t* const cand = A.cand;
  load_levels(s_sf, g.sf);

  for (int b = blockIdx.x; b < g.nitems; b += gridDim.x) {
    __syncthreads();                       // the previous item's shared state has been read
    int32_t* const omatch = g.kp_match + (size_t)b * cap;
    int32_t* const oobs = g.kp_obs + (size_t)b * cap;
    const orbx_localmatch_point* const mp = g.mp + (size_t)b * mcap;
    // ---- the check: nothing below addresses memory with a value that was not tested here
    const int f = g.frames[b], nmp = g.nmp[b];
    bool ok = f >= 0 && f < g.nframes && nmp >= 0 && nmp <= mcap;
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
      for (int q = tid; q < nmp; q += kThreads) {
        const uint4 hi = ((const uint4*)(mp + q))[1];
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
    for (int q = tid; q < nmp; q += kThreads) res[q] = -1;
    build_grid<kThreads>(G, kp, g.uright ? g.uright + of : nullptr, n, A, [&](int i) { if (oobs[i] > 0) set_bit(s_hidden, i); });

    // ---- phase A: every point's candidate count, then the offsets
    for (int q = tid; q <= nmp; q += kThreads) {
      int c = 0;
      if (q < nmp) {
        const Pt t = load_point(mp + q, s_sf, g.th, g.factor);
        if (t.live)
          walk<true>(G, t.x, t.y, t.radius, t.level - 1, t.level, A, [&](const Rec& r, int) {
            if (r.ur > 0.0f && fabsf(t.xr - r.ur) > t.radius) return;   // the stereo gate, src/ORBmatcher.cc:96-101
            c++;
          });
      }
      offs[q] = c;
    }
    scan_offsets<kThreads>(offs, nmp + 1);
    if (LDS) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the LDS-DMA loads have landed
    __syncthreads();

    // ---- chunks of points whose candidates fit the room: lists with distances (all waves), then the chain (wave 0)
    int nm = 0;                            // wave 0's count of acceptances
    for (int q0 = 0; q0 < nmp;) {
      const int e0 = offs[q0], q1 = chunk_end(offs, q0, nmp, g.room);
      const int tot = min(offs[q1] - e0, g.room);
      for (int q = q0 + tid; q < q1; q += kThreads) {
        int k = offs[q] - e0;
        const int kend = offs[q + 1] - e0;
        if (kend > k) {
          const Pt t = load_point(mp + q, s_sf, g.th, g.factor);
          const D8 qd = load_desc(g.pdesc + (size_t)t.point * 32);   // the pool row is below npoints: the check
          walk<true>(G, t.x, t.y, t.radius, t.level - 1, t.level, A, [&](const Rec& r, int i) {
            if (r.ur > 0.0f && fabsf(t.xr - r.ur) > t.radius) return;
            if (k < kend && k < tot) {
              const int d = hamming(qd, load_desc(desc + (size_t)i * 32));
              cand[k] = (uint32_t)i | (uint32_t)d << 15 | ((uint32_t)r.octave & 31u) << 24;
            }
            k++;
          });
        }
      }
      __syncthreads();

#ifndef ORBX_LOCALMATCH_NO_CHAIN          // (a timing build without phase B: tools/localmatch_times.py; its results are not the specification's)
      if (tid < 64) {                      // ---- phase B
        for (int c0 = q0; c0 < q1; c0 += 64) {
          const int cn = min(64, q1 - c0);
          int l_b = 0, l_n = 0, l_obs = 0;
          if (lane < cn) {
            l_b = offs[c0 + lane] - e0; l_n = offs[c0 + lane + 1] - e0 - l_b;
            l_obs = mp[c0 + lane].obs;
          }
          for (int i = 0; i < cn; i++) {
            const int cnt = __builtin_amdgcn_readlane(l_n, i);
            if (cnt <= 0) continue;
            const int b0 = __builtin_amdgcn_readlane(l_b, i);
            int k1 = kNone, k2 = kNone;    // the lane's two smallest (distance << 15 | position)
            for (int j = lane; j < cnt; j += 64) {
              const uint32_t e = cand[b0 + j];
              const int idx = (int)(e & 0x7FFFu);
              if ((ld(s_hidden + (idx >> 5)) >> (idx & 31)) & 1) continue;
              const int key = (int)((e >> 15) & 0x1FFu) << 15 | j;
              const int hi = max(k1, key);
              k1 = min(k1, key);
              k2 = min(k2, hi);
            }
            const int m1 = wave_min(k1);
            if (m1 == kNone || (m1 >> 15) > kThHigh) continue;
            const int m2 = wave_min(k1 == m1 ? k2 : k1);   // positions are unique: one lane holds m1
            const uint32_t e1 = cand[b0 + (m1 & 0x7FFF)];
            const int best = m1 >> 15, level1 = (int)(e1 >> 24 & 31u);
            int second = 256, level2 = 31; // bestDist2 = 256, bestLevel2 = -1
            if (m2 != kNone) {
              second = m2 >> 15;
              level2 = (int)(cand[b0 + (m2 & 0x7FFF)] >> 24 & 31u);
            }
            // :117-130: dropped when the levels agree and bestDist > mfNNratio * bestDist2, kept when they differ or bestDist <= ...
            if (level1 != level2 || (float)best <= g.ratio * (float)second) {
              const int obs = __builtin_amdgcn_readlane(l_obs, i);
              if (lane == 0) {
                const int idx = (int)(e1 & 0x7FFFu);
                st(res + c0 + i, idx);
                if (obs > 0) st(s_hidden + (idx >> 5), ld(s_hidden + (idx >> 5)) | (int)(1u << (idx & 31)));
              }
              nm++;
              __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // the stores are done before the next point's loads
            }
          }
        }
      }
#endif
      __syncthreads();
      q0 = q1;
    }

    // ---- phase C: the last point that took a keypoint holds it; integer maxima, so the order does not matter
    for (int q = tid; q < nmp; q += kThreads) {
      const int i = res[q];
      if (i >= 0 && i < n) __hip_atomic_fetch_max(omatch + i, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    for (int i = tid; i < n; i += kThreads) {
      const int q = __hip_atomic_load(omatch + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (q >= 0 && q < nmp) oobs[i] = mp[q].obs;
    }
    if (tid == 0) g.nmatches[b] = nm;
  }
}

// what both forms check before anything is copied or launched
int check(orbx_localmatch* m, const char* who, const orbx_localmatch_side* side, const void* frames, int nitems, const void* mp, const void* nmp,
          int mcap, const void* pdesc, int npoints, const float* sf, int nlevels, float th, const void* kp_obs, const void* kp_match,
          const void* nmatches) {
  return check_call(m, who, side, frames && mp && nmp && pdesc, "frames, map points, nmp or pdesc", kp_obs && kp_match && nmatches,
                    "kp_obs, kp_match or nmatches", nitems, mcap, npoints, sf, nlevels, std::isfinite(th) ? nullptr : "th must be finite");
}

}  // namespace

extern "C" {

int orbx_localmatch_create(orbx_localmatch** out, int device) {
  return create_handle(out, device, "orbx_localmatch_create", orbx_localmatch_destroy,
                       [](orbx_localmatch* m) { return open_window(m, "ORBX_LOCALMATCH_LDS", (const void*)k_local_match<true>); });
}

void orbx_localmatch_destroy(orbx_localmatch* m) { destroy_handle(m); }

const char* orbx_localmatch_last_error(const orbx_localmatch* m) { return last_error(m); }

int orbx_localmatch_search_device(orbx_localmatch* m, const orbx_localmatch_side* side, const int32_t* d_frames, int nitems,
                                  const orbx_localmatch_point* d_mp, const int32_t* d_nmp, int mcap, const uint8_t* d_pdesc, int npoints,
                                  const float* scale_factors, int nlevels, float th, float nn_ratio, int32_t* d_kp_obs, int32_t* d_kp_match,
                                  int32_t* d_nmatches, void* stream) {
  if (!m) return ORBX_E_INVALID;
  const char* who = "orbx_localmatch_search_device: ";
  int rc = check(m, who, side, d_frames, nitems, d_mp, d_nmp, mcap, d_pdesc, npoints, scale_factors, nlevels, th, d_kp_obs, d_kp_match, d_nmatches);
  if (rc != ORBX_OK) return rc;
  if (((uintptr_t)side->d_desc | (uintptr_t)d_mp | (uintptr_t)d_pdesc) & 15)
    return fail(m, ORBX_E_INVALID, std::string(who) + "d_desc, d_mp and d_pdesc must be 16-byte aligned");
  rc = same_device(m, who, {side->d_kps, side->d_desc, side->d_counts, side->d_uright, side->d_bounds, d_frames, d_mp, d_nmp, d_pdesc, d_kp_obs,
                            d_kp_match, d_nmatches}, "the handle");
  if (rc != ORBX_OK) return rc;
  ORBX_SIDE_HIP(m, hipSetDevice(m->device));
  const int cap = side->capacity;
  int p2;
  Paths path;
  if ((rc = plan(m, cap, mcap, nitems, &p2, &path)) != ORBX_OK) return rc;
  Args g;
  g.kps = (const uint8_t*)side->d_kps; g.desc = side->d_desc; g.counts = side->d_counts; g.uright = side->d_uright; g.bounds = side->d_bounds;
  g.frames = d_frames; g.mp = d_mp; g.nmp = d_nmp; g.pdesc = d_pdesc;
  g.kp_obs = d_kp_obs; g.kp_match = d_kp_match; g.nmatches = d_nmatches;
  g.scratch = path.in_lds ? nullptr : m->scratch.p; g.scratch_stride = path.scratch_stride;
  g.nframes = side->nframes; g.cap = cap; g.nitems = nitems; g.mcap = mcap; g.npoints = npoints; g.nlevels = nlevels; g.p2 = p2; g.room = path.room;
  g.factor = (double)th != 1.0;            // bFactor, src/ORBmatcher.cc:48
  g.th = th; g.ratio = nn_ratio;
  fill_levels(g.sf, scale_factors, nlevels);
  hipStream_t st = stream ? (hipStream_t)stream : m->st;
  if ((rc = wait_previous(m, st)) != ORBX_OK) return rc;
  if (path.in_lds) hipLaunchKernelGGL(k_local_match<true>, dim3((unsigned)path.blocks), dim3(kThreads), path.lds_bytes, st, g);
  else hipLaunchKernelGGL(k_local_match<false>, dim3((unsigned)path.blocks), dim3(kThreads), 0, st, g);
  return record_call(m, st);
}

int orbx_localmatch_search(orbx_localmatch* m, const orbx_localmatch_side* side, const int32_t* frames, int nitems,
                           const orbx_localmatch_point* mp, const int32_t* nmp, int mcap, const uint8_t* pdesc, int npoints,
                           const float* scale_factors, int nlevels, float th, float nn_ratio, int32_t* kp_obs, int32_t* kp_match,
                           int32_t* nmatches) {
  if (!m) return ORBX_E_INVALID;
  const char* who = "orbx_localmatch_search: ";
  int rc = check(m, who, side, frames, nitems, mp, nmp, mcap, pdesc, npoints, scale_factors, nlevels, th, kp_obs, kp_match, nmatches);
  if (rc != ORBX_OK) return rc;
  Stager io;
  const size_t nf = (size_t)side->nframes, nk = nf * side->capacity, rows = (size_t)nitems * side->capacity;
  const size_t o_kps = io.in(side->d_kps, nk * sizeof(orbx_keypoint)), o_desc = io.in(side->d_desc, nk * 32), o_counts = io.in(side->d_counts, nf * 8);
  const size_t o_ur = side->d_uright ? io.in(side->d_uright, nk * 4) : 0, o_bounds = io.in(side->d_bounds, nf * 16);
  const size_t o_frames = io.in(frames, (size_t)nitems * 4), o_mp = io.in(mp, (size_t)nitems * mcap * sizeof(orbx_localmatch_point));
  const size_t o_nmp = io.in(nmp, (size_t)nitems * 4), o_pdesc = io.in(pdesc, (size_t)npoints * 32);
  const size_t o_obs = io.out(kp_obs, rows * 4, true), o_match = io.out(kp_match, rows * 4), o_nm = io.out(nmatches, (size_t)nitems * 4);
  if ((rc = upload(m, io)) != ORBX_OK) return rc;
  uint8_t* const d = m->io.p;
  const orbx_localmatch_side ds = {(const orbx_keypoint*)(d + o_kps), d + o_desc, (const int32_t*)(d + o_counts),
                                   side->d_uright ? (const float*)(d + o_ur) : nullptr, (const float*)(d + o_bounds), side->nframes, side->capacity};
  rc = orbx_localmatch_search_device(m, &ds, (const int32_t*)(d + o_frames), nitems, (const orbx_localmatch_point*)(d + o_mp),
                                     (const int32_t*)(d + o_nmp), mcap, d + o_pdesc, npoints, scale_factors, nlevels, th, nn_ratio,
                                     (int32_t*)(d + o_obs), (int32_t*)(d + o_match), (int32_t*)(d + o_nm), m->st);
  if (rc != ORBX_OK) return rc;
  return download(m, io);
}

}  // extern "C"
