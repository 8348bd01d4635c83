// The two-camera rig blocks of Tracking's two projection matchers, batched (include/orbx_rigmatch.h): SearchLocalPoints
// (src/ORBmatcher.cc:43-212) and SearchByProjection(CurrentFrame, LastFrame) (:1676-1886), both with Nleft != -1, for B items on the left
// and right extractions and the left/right match tables a batched rig front-end left in HBM.
//
// k_rig_match<LDS, LAST>: one workgroup of 8 waves per item (a grid of at most kMaxBlocks workgroups walks the items).  The frame grid, the
// window walk, the offsets' scan, the chunk cut, the chain's step (the scan over the open candidates, the ratio test, the bind), the last
// writer, the rotation filter and the layout are csrc/side/orbx_window_device.h's, the grid used twice: a left and a right one in two
// Arrays that share the offsets, the results and the candidate room.  This file holds what is the rig's own:
//   check                the item's frame, both counts, the row's count and every in-view point's levels and pool row, the match tables'
//                        entries (entry 1), the direction and th (entry 2), before any of them addresses memory.
//   phase A              a LIST PER (POINT, CAMERA), list 2 q + camera: the window over that camera's grid; a candidate is one word: index
//                        in its camera (15 bits), Hamming distance (9), octave (5, two's complement).  The distances depend on nothing in
//                        the chain.  Chunks are cut between points, never between a point's two lists: the room holds at least
//                        cap_l + cap_r candidates.
//   phase B, wave 0      the walk over the chunk's points in index order: the left sub-step, then the right sub-step, each the core's step on
//                        its list (a bit per slot in LDS, right slots at cap_l + index).  Every bind sets or clears the slot's hidden bit by
//                        the writer's obs, so the right sub-step sees what the left one of the same point bound (entry 1's l2r binding).
//                        The :126 and :1735 exits are wave-uniform.  A point records up to four (entry 1) or two (entry 2) slots.
//   phase C, all waves   the core's last writer over those results.
//   phase D, all waves   entry 2 under check_orientation: the core's rotation filter over both results of every point (the left or the right
//                        keypoint's angle by the slot); kp_match = -2, kp_obs = -1 for every entry of another bin.
// The hidden bits are 4 KiB of static LDS on both paths.
// The float expressions are compiled with -ffp-contract=off: every operation is rounded by itself, as the specification states them.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../side/orbx_handle.h"
#include "../side/orbx_pair_device.h"
#include "../side/orbx_window_device.h"
#include "../side/orbx_window_host.h"
#include "../../../include/orbx_rigmatch.h"

#ifdef ORBX_RIGMATCH_NO_CHAIN
#warning "ORBX_RIGMATCH_NO_CHAIN: a timing build without phase B; its results are not the specification's"
#endif

struct orbx_rigmatch : orbx::side::win::WindowHandle {};   // lds_limit: ORBX_RIGMATCH_LDS at create

namespace {

using namespace orbx::side;
using namespace orbx::side::dev;
using namespace orbx::side::win;

constexpr int kRowBytes = 48;             // both entries' point rows
static_assert(ORBX_RIGMATCH_MAX_CAPACITY == kMaxCap && ORBX_RIGMATCH_MAX_LEVELS == kMaxLevels, "the window core's limits");
static_assert(sizeof(orbx_rigmatch_local_point) == kRowBytes && sizeof(orbx_rigmatch_last_point) == kRowBytes, "three 16-byte loads a row");
static_assert(sizeof(orbx_rigmatch_last_item) == 16, "the item");

struct Args {
  const uint8_t* kps_l; const uint8_t* desc_l; const int32_t* counts_l;
  const uint8_t* kps_r; const uint8_t* desc_r; const int32_t* counts_r;
  const int32_t* l2r; const int32_t* r2l; const float* bounds;
  const int32_t* frames; const orbx_rigmatch_last_item* items;   // entry 1 resp. entry 2
  const uint8_t* rows; const int32_t* nrows; const uint8_t* pdesc;
  int32_t* kp_obs; int32_t* kp_match; int32_t* nmatches;
  uint8_t* scratch; size_t scratch_stride;
  int nframes, cap_l, cap_r, nitems, mcap, npoints, nlevels, p2l, p2r, room, factor, check_ori;
  float th, ratio;
  float sf[kMaxLevels];
};

// a (point, camera) window
struct Pt { float x, y, radius; int lo, hi, point; bool live; };

// entry 1's row {proj_x, proj_y, view_cos, level | proj_xr, proj_yr, view_cos_r, level_r | obs, point, in_view, in_view_r}:
// RadiusByViewingCos (src/ORBmatcher.cc:214-220); th on the left camera alone (:68, :147); levels (level - 1, level)
__device__ __forceinline__ Pt load_local(const uint8_t* row, int cam, const float* s_sf, float th, int factor) {
  const uint4* const rp = (const uint4*)row;
  const uint4 a = rp[cam], c = rp[2];
  Pt t;
  t.x = __uint_as_float(a.x); t.y = __uint_as_float(a.y);
  const float vc = __uint_as_float(a.z);
  const int level = (int)a.w;
  t.point = (int)c.y;
  // in view, and finite: a NaN fails every comparison (the reference leaves a non-finite projection undefined; here it has no candidate)
  t.live = (cam ? c.w != 0u && level != -1 : c.z != 0u) && fabsf(t.x) < INFINITY && fabsf(t.y) < INFINITY && fabsf(vc) < INFINITY;
  t.radius = 0.0f; t.lo = 0; t.hi = 0;
  if (t.live) {                            // the level is one of the table's: the check
    float r = ((double)vc > 0.998) ? 2.5f : 4.0f;
    if (factor && !cam) r *= th;
    t.radius = r * s_sf[level];
    t.lo = level - 1; t.hi = level;
  }
  return t;
}

// entry 2's row {u, v, u_r, v_r | angle, octave, obs, point | valid, -}: th times the octave's scale (:1724, :1802), the direction's level
// range (:1728-1733, :1806-1811)
__device__ __forceinline__ Pt load_last(const uint8_t* row, int cam, const float* s_sf, float th, int direction) {
  const uint4* const rp = (const uint4*)row;
  const uint4 a = rp[0], b = rp[1], c = rp[2];
  Pt t;
  t.x = __uint_as_float(cam ? a.z : a.x); t.y = __uint_as_float(cam ? a.w : a.y);
  const int octave = (int)b.y;
  t.point = (int)b.w;
  t.live = c.x != 0u && fabsf(t.x) < INFINITY && fabsf(t.y) < INFINITY;
  t.radius = 0.0f; t.lo = 0; t.hi = 0;
  if (t.live) {                            // the octave is one of the table's: the check
    t.radius = th * s_sf[octave];
    if (direction == 1) { t.lo = octave; t.hi = -1; }
    else if (direction == 2) { t.lo = 0; t.hi = octave; }
    else { t.lo = octave - 1; t.hi = octave + 1; }
  }
  return t;
}

template <bool LDS, bool LAST>
__global__ __launch_bounds__(kThreads) void k_rig_match(Args g) {
  extern __shared__ __align__(16) uint8_t smem[];
  __shared__ int s_bad;
  __shared__ int32_t s_hidden[kMaxCap / 32];   // bit s: slot s holds a map point with Observations() > 0
  __shared__ float s_sf[kMaxLevels];
  constexpr int RES = LAST ? 2 : 4;            // results a point
  const int tid = threadIdx.x, lane = tid & 63;
  const int cap_l = g.cap_l, cap_r = g.cap_r, slots = cap_l + cap_r, mcap = g.mcap;
  const RigLay L = rig_layout(cap_l, cap_r, mcap, g.p2l, g.p2r, LDS);
  uint8_t* const base = LDS ? smem : g.scratch + (size_t)blockIdx.x * g.scratch_stride;
  const Arrays AL = arrays(base, L, L.grid_l), AR = arrays(base, L, L.grid_r);
  int32_t *const offs = AL.offs, *const res = AL.res;
  uint32_t* const cand = AL.cand;
  load_levels(s_sf, g.sf);

  for (int b = blockIdx.x; b < g.nitems; b += gridDim.x) {
    __syncthreads();                       // the previous item's shared state has been read
    int32_t* const omatch = g.kp_match + (size_t)b * slots;
    int32_t* const oobs = g.kp_obs + (size_t)b * slots;
    const uint8_t* const rows = g.rows + (size_t)b * mcap * kRowBytes;
    // ---- the check: nothing below addresses memory with a value that was not tested here
    int f, direction = 0;
    float th = g.th;
    bool ok = true;
    if (LAST) {
      f = g.items[b].frame; direction = g.items[b].direction; th = g.items[b].th;
      ok = direction >= 0 && direction <= 2 && fabsf(th) < INFINITY;
    } else {
      f = g.frames[b];
    }
    const int nq = g.nrows[b];
    ok = ok && f >= 0 && f < g.nframes && nq >= 0 && nq <= mcap;
    int nl = 0, nr = 0;
    if (ok) {
      nl = g.counts_l[2 * f]; nr = g.counts_r[2 * f];
      ok = nl >= 0 && nl <= cap_l && nr >= 0 && nr <= cap_r;
    }
    if (tid == 0) s_bad = 0;
    for (int i = tid; i < slots; i += kThreads) omatch[i] = -1;
    __syncthreads();
    if (ok) {                              // uniform over the workgroup
      bool bad = false;
      for (int q = tid; q < nq; q += kThreads) {
        const uint4* const rp = (const uint4*)(rows + (size_t)q * kRowBytes);
        if (LAST) {
          const uint4 r1 = rp[1], r2 = rp[2];
          bad |= r2.x != 0u && ((int)r1.y < 0 || (int)r1.y >= g.nlevels || (int)r1.w < 0 || (int)r1.w >= g.npoints);
        } else {
          const uint4 r0 = rp[0], r1 = rp[1], r2 = rp[2];
          const bool in_l = r2.z != 0u, in_r = r2.w != 0u;
          bad |= in_l && ((int)r0.w < 0 || (int)r0.w >= g.nlevels);
          bad |= in_r && ((int)r1.w < -1 || (int)r1.w >= g.nlevels);
          bad |= (in_l || in_r) && ((int)r2.y < 0 || (int)r2.y >= g.npoints);
        }
      }
      if (!LAST) {
        for (int i = tid; i < nl; i += kThreads) { const int v = g.l2r[(size_t)f * cap_l + i]; bad |= v < -1 || v >= nr; }
        for (int i = tid; i < nr; i += kThreads) { const int v = g.r2l[(size_t)f * cap_r + i]; bad |= v < -1 || v >= nl; }
      }
      if (bad) s_bad = 1;
    }
    __syncthreads();
    if (!ok || s_bad) {                    // uniform over the workgroup: a row of -1, kp_obs as it was
      if (tid == 0) g.nmatches[b] = -1;
      continue;
    }
    const size_t ofl = (size_t)f * cap_l, ofr = (size_t)f * cap_r;
    const uint8_t* const kpl = g.kps_l + ofl * sizeof(orbx_keypoint);
    const uint8_t* const kpr = g.kps_r + ofr * sizeof(orbx_keypoint);
    const uint8_t* const descl = LDS ? base + L.desc_l : g.desc_l + ofl * 32;
    const uint8_t* const descr = LDS ? base + L.desc_r : g.desc_r + ofr * 32;
    const Grid G = frame_grid(g.bounds + 4 * f);
    auto load = [&](int q, int cam) {
      const uint8_t* const row = rows + (size_t)q * kRowBytes;
      return LAST ? load_last(row, cam, s_sf, th, direction) : load_local(row, cam, s_sf, th, g.factor);
    };
    auto obs_of = [&](int q) { return *(const int32_t*)(rows + (size_t)q * kRowBytes + (LAST ? 24 : 32)); };

    // ---- phase A: both grids, the hidden bits over both slot ranges in the same trips over the keypoints
    if (LDS) {
      stage_dma<kThreads>(base + L.desc_l, g.desc_l + ofl * 32, nl * 2);
      stage_dma<kThreads>(base + L.desc_r, g.desc_r + ofr * 32, nr * 2);
    }
    for (int w = tid; w < kMaxCap / 32; w += kThreads) s_hidden[w] = 0;
    for (int e = tid; e < RES * nq; e += kThreads) res[e] = -1;
    build_grid<kThreads>(G, kpl, nullptr, nl, AL, [&](int i) { if (oobs[i] > 0) set_bit(s_hidden, i); });
    build_grid<kThreads>(G, kpr, nullptr, nr, AR, [&](int i) { if (oobs[cap_l + i] > 0) set_bit(s_hidden, cap_l + i); });

    // ---- phase A: every list's candidate count, then the offsets
    const int nlists = 2 * nq;
    for (int p = tid; p <= nlists; p += kThreads) {
      int c = 0;
      if (p < nlists) {
        const Pt t = load(p >> 1, p & 1);
        if (t.live) walk<!LAST>(G, t.x, t.y, t.radius, t.lo, t.hi, (p & 1) ? AR : AL, [&](const Rec&, int) { c++; });
      }
      offs[p] = c;
    }
    scan_offsets<kThreads>(offs, nlists + 1);
    if (LDS) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the LDS-DMA loads have landed
    __syncthreads();

    // ---- chunks of points whose candidates fit the room: lists with distances (all waves), then the chain (wave 0)
    int nm = 0;                            // wave 0's count of bindings
    for (int q0 = 0; q0 < nq;) {
      const int e0 = offs[2 * q0], q1 = chunk_end<2>(offs, q0, nq, g.room);
      const int tot = min(offs[2 * q1] - e0, g.room);
      for (int p = 2 * q0 + tid; p < 2 * q1; p += kThreads) {
        int k = offs[p] - e0;
        const int kend = offs[p + 1] - e0;
        if (kend > k) {
          const int cam = p & 1;
          const Pt t = load(p >> 1, cam);
          const D8 qd = load_desc(g.pdesc + (size_t)t.point * 32);   // the pool row is below npoints: the check
          const uint8_t* const desc = cam ? descr : descl;
          walk<!LAST>(G, t.x, t.y, t.radius, t.lo, t.hi, cam ? AR : AL, [&](const Rec& r, int i) {
            if (k < kend && k < tot) {
              const int d = hamming(qd, load_desc(desc + (size_t)i * 32));
              cand[k] = (uint32_t)i | (uint32_t)d << 15 | ((uint32_t)r.octave & 31u) << 24;
            }
            k++;
          });
        }
      }
      __syncthreads();

#ifndef ORBX_RIGMATCH_NO_CHAIN           // (a timing build without phase B: tools/rigmatch_times.py; its results are not the specification's)
      if (tid < 64) {                      // ---- phase B
        for (int c0 = q0; c0 < q1; c0 += 64) {
          const int cn = min(64, q1 - c0);
          int l_bl = 0, l_nl = 0, l_br = 0, l_nr = 0, l_obs = 0;
          if (lane < cn) {
            const int q = c0 + lane;
            l_bl = offs[2 * q] - e0; l_br = offs[2 * q + 1] - e0; l_nl = l_br - l_bl; l_nr = offs[2 * q + 2] - e0 - l_br;
            l_obs = obs_of(q);
          }
          for (int i = 0; i < cn; i++) {
            const int cnt_l = __builtin_amdgcn_readlane(l_nl, i), cnt_r = __builtin_amdgcn_readlane(l_nr, i);
            if (cnt_l <= 0 && (LAST || cnt_r <= 0)) continue;   // entry 2: an empty left list ends the point (:1735)
            const int bl = __builtin_amdgcn_readlane(l_bl, i), br = __builtin_amdgcn_readlane(l_br, i);
            const int obs = __builtin_amdgcn_readlane(l_obs, i);
            int32_t* const out = res + (size_t)(c0 + i) * RES;
            LaneKeys mine;
            int m1, idx = 0;
            if (LAST) {
              m1 = open_top(cand, bl, cnt_l, 0, s_hidden, lane);
              if (m1 != kNone && (m1 >> 15) <= kThHigh) {        // :1770
                if (lane == 0) bind<true>(s_hidden, out, (int)(cand[bl + (m1 & 0x7FFF)] & 0x7FFFu), obs);
                nm++;
                publish();
              }
              if (cnt_r <= 0) continue;
              m1 = open_top(cand, br, cnt_r, cap_l, s_hidden, lane);
              if (m1 != kNone && (m1 >> 15) <= kThHigh) {        // :1836
                if (lane == 0) bind<true>(s_hidden, out + 1, cap_l + (int)(cand[br + (m1 & 0x7FFF)] & 0x7FFFu), obs);
                nm++;
                publish();
              }
            } else {
              if (cnt_l > 0) {
                m1 = open_top(cand, bl, cnt_l, 0, s_hidden, lane, &mine);
                const int m2 = (m1 >> 15) <= kThHigh ? open_second(mine, m1) : kNone;
                const int rc = ratio_test(cand, bl, m1, m2, g.ratio, &idx);
                if (rc == 1) continue;     // :126: the point is done, its right block too
                if (rc == 2) {
                  const int x = g.l2r[ofl + idx];   // idx < nl; the entry lies in [-1, nr): the check
                  if (lane == 0) {
                    bind<true>(s_hidden, out, idx, obs);
                    if (x >= 0) bind<true>(s_hidden, out + 1, cap_l + x, obs);   // :131-135, whatever the slot held
                  }
                  nm += 1 + (x >= 0);
                  publish();               // the right block sees these
                }
              }
              if (cnt_r <= 0) continue;
              m1 = open_top(cand, br, cnt_r, cap_l, s_hidden, lane, &mine);
              const int m2 = (m1 >> 15) <= kThHigh ? open_second(mine, m1) : kNone;
              const int rc = ratio_test(cand, br, m1, m2, g.ratio, &idx);
              if (rc >= 2) {               // :193-208: everything but the `continue`
                const int x = g.r2l[ofr + idx];
                if (lane == 0) {
                  if (x >= 0) bind<true>(s_hidden, out + 2, x, obs);             // :198-202
                  bind<true>(s_hidden, out + 3, cap_l + idx, obs);
                }
                nm += 1 + (x >= 0);
                publish();
              }
            }
          }
        }
      }
#endif
      __syncthreads();
      q0 = q1;
    }

    last_writer<kThreads, RES>(res, nq, slots, omatch, oobs, obs_of);   // ---- phase C
    int removed = 0;
    // ---- phase D: the rotation histogram (:1775-1792, :1840-1856), its three maxima and the removal (:1864-1884)
    if (LAST && g.check_ori)               // uniform over the grid; its first barrier: phase C's reads of kp_match and writes of kp_obs are done
      removed = rotation_filter<kThreads, RES>(
          res, nq, slots, [&](int q) { return *(const float*)(rows + (size_t)q * kRowBytes + 16); },
          [&](int s) { return s < cap_l ? kp_field<float>(kpl, s, kAngle) : kp_field<float>(kpr, s - cap_l, kAngle); },   // a written slot is below its count
          [&](int s) { omatch[s] = -2; oobs[s] = -1; });   // entries of one slot write the same values
    if (tid == 0) g.nmatches[b] = nm - removed;
  }
}

// what the window core's checks read of a side: the rig's left buffers and its slots
struct Slots { const void *d_kps, *d_desc, *d_counts, *d_bounds; int nframes, capacity; };

// what all four forms check before anything is copied or launched
int check(orbx_rigmatch* m, const char* who, const orbx_rigmatch_side* side, bool tables, bool inputs, const char* in_names, bool outputs, int nitems,
          int mcap, int npoints, const float* sf, int nlevels, const char* own) {
  if (!side) return fail(m, ORBX_E_INVALID, std::string(who) + "null side");
  if (side->cap_l < 1 || side->cap_r < 1) return fail(m, ORBX_E_INVALID, std::string(who) + "cap_l and cap_r must be at least 1");
  if ((long long)side->cap_l + side->cap_r > (long long)kMaxCap) return fail(m, ORBX_E_INVALID, std::string(who) + "cap_l + cap_r above 32768");
  if (!side->d_kps_r || !side->d_desc_r || !side->d_counts_r || (tables && (!side->d_l2r || !side->d_r2l)))
    return fail(m, ORBX_E_INVALID, std::string(who) + "null buffer in the side");
  const Slots s = {side->d_kps_l, side->d_desc_l, side->d_counts_l, side->d_bounds, side->nframes, side->cap_l + side->cap_r};
  return check_call(m, who, &s, inputs, in_names, outputs, "kp_obs, kp_match or nmatches", nitems, mcap, npoints, sf, nlevels, own);
}

template <bool LAST>
int launch(orbx_rigmatch* m, const char* who, const orbx_rigmatch_side* side, const void* d_items, int nitems, const void* d_rows, const int32_t* d_nrows,
           int mcap, const uint8_t* d_pdesc, int npoints, const float* scale_factors, int nlevels, float th, float nn_ratio, int check_orientation,
           int32_t* d_kp_obs, int32_t* d_kp_match, int32_t* d_nmatches, void* stream) {
  if (((uintptr_t)side->d_desc_l | (uintptr_t)side->d_desc_r | (uintptr_t)d_rows | (uintptr_t)d_pdesc) & 15)
    return fail(m, ORBX_E_INVALID, std::string(who) + "d_desc_l, d_desc_r, the point rows and d_pdesc must be 16-byte aligned");
  int rc = same_device(m, who, {side->d_kps_l, side->d_desc_l, side->d_counts_l, side->d_kps_r, side->d_desc_r, side->d_counts_r, side->d_l2r,
                                side->d_r2l, side->d_bounds, d_items, d_rows, d_nrows, d_pdesc, d_kp_obs, d_kp_match, d_nmatches}, "the handle");
  if (rc != ORBX_OK) return rc;
  ORBX_SIDE_HIP(m, hipSetDevice(m->device));
  const int cap_l = side->cap_l, cap_r = side->cap_r;
  const int p2l = sort_size(cap_l), p2r = sort_size(cap_r);
  Paths path;                              // one point's longest pair of lists is cap_l + cap_r candidates
  rc = plan(m, rig_layout(cap_l, cap_r, mcap, p2l, p2r, true).fixed, rig_layout(cap_l, cap_r, mcap, p2l, p2r, false).fixed, cap_l + cap_r, nitems, &path);
  if (rc != ORBX_OK) return rc;
  Args g;
  g.kps_l = (const uint8_t*)side->d_kps_l; g.desc_l = side->d_desc_l; g.counts_l = side->d_counts_l;
  g.kps_r = (const uint8_t*)side->d_kps_r; g.desc_r = side->d_desc_r; g.counts_r = side->d_counts_r;
  g.l2r = side->d_l2r; g.r2l = side->d_r2l; g.bounds = side->d_bounds;
  g.frames = LAST ? nullptr : (const int32_t*)d_items; g.items = LAST ? (const orbx_rigmatch_last_item*)d_items : nullptr;
  g.rows = (const uint8_t*)d_rows; g.nrows = d_nrows; g.pdesc = d_pdesc;
  g.kp_obs = d_kp_obs; g.kp_match = d_kp_match; g.nmatches = d_nmatches;
  g.nframes = side->nframes; g.cap_l = cap_l; g.cap_r = cap_r; g.nitems = nitems; g.mcap = mcap; g.npoints = npoints; g.nlevels = nlevels;
  g.p2l = p2l; g.p2r = p2r;
  g.factor = (double)th != 1.0;            // bFactor, src/ORBmatcher.cc:47
  g.check_ori = check_orientation != 0;
  g.th = th; g.ratio = nn_ratio;
  fill_levels(g.sf, scale_factors, nlevels);
  return win::launch(m, path, g, k_rig_match<true, LAST>, k_rig_match<false, LAST>, stream);
}

// a host form's side in the handle's io block: two cameras and the tables
struct RigStaged { size_t kl, dl, cl, kr, dr, cr, l2r, r2l, bounds; };
RigStaged stage_side(Stager& io, const orbx_rigmatch_side* s, bool tables) {
  const size_t nf = (size_t)s->nframes, nkl = nf * s->cap_l, nkr = nf * s->cap_r;
  RigStaged o;
  o.kl = io.in(s->d_kps_l, nkl * sizeof(orbx_keypoint)); o.dl = io.in(s->d_desc_l, nkl * 32); o.cl = io.in(s->d_counts_l, nf * 8);
  o.kr = io.in(s->d_kps_r, nkr * sizeof(orbx_keypoint)); o.dr = io.in(s->d_desc_r, nkr * 32); o.cr = io.in(s->d_counts_r, nf * 8);
  o.l2r = tables ? io.in(s->d_l2r, nkl * 4) : 0; o.r2l = tables ? io.in(s->d_r2l, nkr * 4) : 0;
  o.bounds = io.in(s->d_bounds, nf * 16);
  return o;
}
orbx_rigmatch_side device_side(uint8_t* d, const RigStaged& o, const orbx_rigmatch_side* s, bool tables) {
  return {(const orbx_keypoint*)(d + o.kl), d + o.dl, (const int32_t*)(d + o.cl), (const orbx_keypoint*)(d + o.kr), d + o.dr,
          (const int32_t*)(d + o.cr), tables ? (const int32_t*)(d + o.l2r) : nullptr, tables ? (const int32_t*)(d + o.r2l) : nullptr,
          (const float*)(d + o.bounds), s->nframes, s->cap_l, s->cap_r};
}

}  // namespace

extern "C" {

int orbx_rigmatch_create(orbx_rigmatch** out, int device) {
  return create_handle(out, device, "orbx_rigmatch_create", orbx_rigmatch_destroy, [](orbx_rigmatch* m) {
    const char* e = open_window(m, "ORBX_RIGMATCH_LDS", (const void*)k_rig_match<true, false>);
    return e ? e : allow_lds((const void*)k_rig_match<true, true>, kLdsMax);
  });
}

void orbx_rigmatch_destroy(orbx_rigmatch* m) { destroy_handle(m); }

const char* orbx_rigmatch_last_error(const orbx_rigmatch* m) { return last_error(m); }

int orbx_rigmatch_local_device(orbx_rigmatch* m, const orbx_rigmatch_side* side, const int32_t* d_frames, int nitems,
                               const orbx_rigmatch_local_point* d_mp, const int32_t* d_nmp, int mcap, const uint8_t* d_pdesc, int npoints,
                               const float* scale_factors, int nlevels, float th, float nn_ratio, int32_t* d_kp_obs, int32_t* d_kp_match,
                               int32_t* d_nmatches, void* stream) {
  if (!m) return ORBX_E_INVALID;
  const char* who = "orbx_rigmatch_local_device: ";
  const int rc = check(m, who, side, true, d_frames && d_mp && d_nmp && d_pdesc, "frames, map points, nmp or pdesc", d_kp_obs && d_kp_match && d_nmatches,
                       nitems, mcap, npoints, scale_factors, nlevels, std::isfinite(th) ? nullptr : "th must be finite");
  if (rc != ORBX_OK) return rc;
  return launch<false>(m, who, side, d_frames, nitems, d_mp, d_nmp, mcap, d_pdesc, npoints, scale_factors, nlevels, th, nn_ratio, 0, d_kp_obs,
                       d_kp_match, d_nmatches, stream);
}

int orbx_rigmatch_local(orbx_rigmatch* m, const orbx_rigmatch_side* side, const int32_t* frames, int nitems, const orbx_rigmatch_local_point* mp,
                        const int32_t* nmp, int mcap, const uint8_t* pdesc, int npoints, const float* scale_factors, int nlevels, float th,
                        float nn_ratio, int32_t* kp_obs, int32_t* kp_match, int32_t* nmatches) {
  if (!m) return ORBX_E_INVALID;
  const char* who = "orbx_rigmatch_local: ";
  int rc = check(m, who, side, true, frames && mp && nmp && pdesc, "frames, map points, nmp or pdesc", kp_obs && kp_match && nmatches, nitems, mcap,
                 npoints, scale_factors, nlevels, std::isfinite(th) ? nullptr : "th must be finite");
  if (rc != ORBX_OK) return rc;
  Stager io;
  const size_t rows = (size_t)nitems * (side->cap_l + side->cap_r);
  const RigStaged ss = stage_side(io, side, true);
  const size_t o_frames = io.in(frames, (size_t)nitems * 4), o_mp = io.in(mp, (size_t)nitems * mcap * kRowBytes);
  const size_t o_nmp = io.in(nmp, (size_t)nitems * 4), o_pdesc = io.in(pdesc, (size_t)npoints * 32);
  const size_t o_obs = io.out(kp_obs, rows * 4, true), o_match = io.out(kp_match, rows * 4), o_nm = io.out(nmatches, (size_t)nitems * 4);
  if ((rc = upload(m, io)) != ORBX_OK) return rc;
  uint8_t* const d = m->io.p;
  const orbx_rigmatch_side ds = device_side(d, ss, side, true);
  rc = orbx_rigmatch_local_device(m, &ds, (const int32_t*)(d + o_frames), nitems, (const orbx_rigmatch_local_point*)(d + o_mp),
                                  (const int32_t*)(d + o_nmp), mcap, d + o_pdesc, npoints, scale_factors, nlevels, th, nn_ratio,
                                  (int32_t*)(d + o_obs), (int32_t*)(d + o_match), (int32_t*)(d + o_nm), m->st);
  if (rc != ORBX_OK) return rc;
  return download(m, io);
}

int orbx_rigmatch_last_device(orbx_rigmatch* m, const orbx_rigmatch_side* side, const orbx_rigmatch_last_item* d_items, int nitems,
                              const orbx_rigmatch_last_point* d_points, const int32_t* d_nlast, int mcap, const uint8_t* d_pdesc, int npoints,
                              const float* scale_factors, int nlevels, int check_orientation, int32_t* d_kp_obs, int32_t* d_kp_match,
                              int32_t* d_nmatches, void* stream) {
  if (!m) return ORBX_E_INVALID;
  const char* who = "orbx_rigmatch_last_device: ";
  const int rc = check(m, who, side, false, d_items && d_points && d_nlast && d_pdesc, "items, points, nlast or pdesc",
                       d_kp_obs && d_kp_match && d_nmatches, nitems, mcap, npoints, scale_factors, nlevels, nullptr);
  if (rc != ORBX_OK) return rc;
  return launch<true>(m, who, side, d_items, nitems, d_points, d_nlast, mcap, d_pdesc, npoints, scale_factors, nlevels, 1.0f, 0.0f,
                      check_orientation, d_kp_obs, d_kp_match, d_nmatches, stream);
}

int orbx_rigmatch_last(orbx_rigmatch* m, const orbx_rigmatch_side* side, const orbx_rigmatch_last_item* items, int nitems,
                       const orbx_rigmatch_last_point* points, const int32_t* nlast, int mcap, const uint8_t* pdesc, int npoints,
                       const float* scale_factors, int nlevels, int check_orientation, int32_t* kp_obs, int32_t* kp_match, int32_t* nmatches) {
  if (!m) return ORBX_E_INVALID;
  const char* who = "orbx_rigmatch_last: ";
  int rc = check(m, who, side, false, items && points && nlast && pdesc, "items, points, nlast or pdesc", kp_obs && kp_match && nmatches, nitems, mcap,
                 npoints, scale_factors, nlevels, nullptr);
  if (rc != ORBX_OK) return rc;
  Stager io;
  const size_t rows = (size_t)nitems * (side->cap_l + side->cap_r);
  const RigStaged ss = stage_side(io, side, false);
  const size_t o_items = io.in(items, (size_t)nitems * sizeof(orbx_rigmatch_last_item)), o_pts = io.in(points, (size_t)nitems * mcap * kRowBytes);
  const size_t o_nlast = io.in(nlast, (size_t)nitems * 4), o_pdesc = io.in(pdesc, (size_t)npoints * 32);
  const size_t o_obs = io.out(kp_obs, rows * 4, true), o_match = io.out(kp_match, rows * 4), o_nm = io.out(nmatches, (size_t)nitems * 4);
  if ((rc = upload(m, io)) != ORBX_OK) return rc;
  uint8_t* const d = m->io.p;
  const orbx_rigmatch_side ds = device_side(d, ss, side, false);
  rc = orbx_rigmatch_last_device(m, &ds, (const orbx_rigmatch_last_item*)(d + o_items), nitems, (const orbx_rigmatch_last_point*)(d + o_pts),
                                 (const int32_t*)(d + o_nlast), mcap, d + o_pdesc, npoints, scale_factors, nlevels, check_orientation,
                                 (int32_t*)(d + o_obs), (int32_t*)(d + o_match), (int32_t*)(d + o_nm), m->st);
  if (rc != ORBX_OK) return rc;
  return download(m, io);
}

}  // extern "C"
