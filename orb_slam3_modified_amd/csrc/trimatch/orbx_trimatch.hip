// The batched SearchForTriangulation (include/orbx_trimatch.h): ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:907-1146, single
// camera, pinhole) for P (keyframe, keyframe) pairs on the descriptors, keypoints and FeatureVectors a batch extraction and
// orbx_bow_transform_batch_device left in HBM.
//
// k_tri_pairs<LDS>: one workgroup of 8 waves per pair (a grid of at most kMaxBlocks workgroups walks the pairs).
//   stage      the two fv_feat lists, each entry with its feature's flags in the top bits (skip: has a point, or not stereo under
//              only_stereo; stereo: uright >= 0); every entry is checked against its frame's count and every listed B feature's octave
//              against nlevels on the way.  LDS path: the lists, the two descriptor sets (16-byte LDS-DMA loads), the work list and the
//              match row in LDS -- 32 (capA + capB) + 16 (min(capA, capB) + capA / 16 + 1) + 4 (2 capA + capB) bytes.  Global path (pairs
//              that need more LDS than the handle's limit): the descriptors where they lie, lists and work list in the workgroup's slice
//              of the handle's scratch, the match row in the caller's d_matches12.
//   intersect  common_nodes (orbx_pair_device.h), a thread per A node: binary search in B's node list; a common node becomes chunks of
//              at most kChunk queries (a0, a1, b0, b1) in a work list.
//   queries    there is no chain (vbMatched2 is never written): all waves take chunks from the list (an LDS counter) and nothing orders them.
//              Lanes take B candidates:
//                nb <= 64: lane j keeps candidate j -- descriptor in 8 registers, flags in one -- over the chunk's queries;
//                larger: a trip loop, lane j scans candidates j, j + 64, ...
//              The A descriptor is wave-uniform.  A lane with dist <= 50 evaluates the two float gates (a, b, c of the epipolar line depend
//              on the query alone) and holds the key dist << 16 | (0xFFFF - position); every other lane holds INT_MAX.  One DPP
//              min-reduction gives the winner: the smallest distance, the LAST position among its holders.
//   filter     after a barrier: a thread per A feature adds its match's bin to an LDS histogram; one lane runs three_maxima; a thread
//              per A feature recomputes its bin, drops the match when the bin lost, writes matches12 and counts.
// The gates are compiled with -ffp-contract=off: every float operation is rounded by itself, as the specification states them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <string>

#include "../side/orbx_handle.h"
#include "../side/orbx_pair_device.h"
#include "../side/orbx_pair_host.h"
#include "../../../include/orbx_trimatch.h"

namespace {

using namespace orbx::side::dev;

constexpr int kThreads = 512;             // 8 waves
constexpr int kChunk = 16;                // queries of one work item
constexpr int kThLow = 50;
constexpr uint32_t kSkip = 0x80000000u, kStereo = 0x40000000u, kIdx = 0x3FFFFFFFu;   // a staged fv_feat entry

struct Side {
  const uint8_t* kps; const uint8_t* desc; const int32_t* counts; const uint32_t* fv_node; const int32_t* fv_ptr; const uint32_t* fv_feat;
  const int32_t* fv_n; const uint8_t* has_point; const float* uright;
  int nframes, cap;
};

struct Args {
  Side a, b;
  const int32_t* pairs; const float* geom;
  int32_t* m12; int32_t* nm;
  uint8_t* scratch; size_t scratch_stride;   // the global path's work list and staged lists, one slice per workgroup
  int npairs, nlevels, only_stereo, coarse, check_ori;
  float scale[ORBX_TRIMATCH_MAX_LEVELS], sigma2[ORBX_TRIMATCH_MAX_LEVELS];
};

__host__ __device__ inline int max_work(int capA, int capB) { return (capA < capB ? capA : capB) + capA / kChunk + 1; }

constexpr size_t kX = offsetof(orbx_keypoint, x), kY = offsetof(orbx_keypoint, y), kAngle = offsetof(orbx_keypoint, angle),
                 kOctave = offsetof(orbx_keypoint, octave);

struct Geom { float f00, f01, f02, f10, f11, f12, f20, f21, f22, epx, epy; };

// gates (2) and (3) of the specification for candidate `fb` of a query at (x1, y1); both_mono: neither feature is stereo
__device__ __forceinline__ bool gates(const Args& g, const Geom& G, const float* s_scale, const float* s_sig, float x1, float y1, const uint8_t* kB,
                                      uint32_t fb, bool both_mono) {
  const float x2 = kp_field<float>(kB, fb, kX), y2 = kp_field<float>(kB, fb, kY);
  const int oct = kp_field<int32_t>(kB, fb, kOctave);   // inside [0, nlevels): checked when the list was staged
  if (both_mono) {
    const float distex = G.epx - x2, distey = G.epy - y2;
    if (distex * distex + distey * distey < 100.0f * s_scale[oct]) return false;
  }
  if (g.coarse) return true;
  const float a = x1 * G.f00 + y1 * G.f10 + G.f20;
  const float b = x1 * G.f01 + y1 * G.f11 + G.f21;
  const float c = x1 * G.f02 + y1 * G.f12 + G.f22;
  const float num = a * x2 + b * y2 + c;
  const float den = a * a + b * b;
  if (den == 0) return false;
  const float dsqr = num * num / den;
  return (double)dsqr < 3.84 * (double)s_sig[oct];
}

__device__ __forceinline__ void fail_row(const Args& g, int p, int32_t* o12) {
  for (int i = threadIdx.x; i < g.a.cap; i += kThreads) o12[i] = -1;
  if (threadIdx.x == 0) g.nm[p] = -1;
}

template <bool LDS>
__global__ __launch_bounds__(kThreads) void k_tri_pairs(Args g) {
  extern __shared__ __align__(16) uint8_t smem[];
  __shared__ int s_cnt, s_next, s_bad, s_nm;
  __shared__ int s_hist[32];
  __shared__ int s_ind[3];
  __shared__ float s_scale[ORBX_TRIMATCH_MAX_LEVELS], s_sig[ORBX_TRIMATCH_MAX_LEVELS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int capA = g.a.cap, capB = g.b.cap, maxw = max_work(capA, capB);
  // LDS: descriptors A | descriptors B | work list | fv_feat A | fv_feat B | match row of A
  // scratch slice: work list | fv_feat A | fv_feat B
  uint8_t* const base = LDS ? smem + (size_t)(capA + capB) * 32 : g.scratch + (size_t)blockIdx.x * g.scratch_stride;
  int4* const work = (int4*)base;
  uint32_t* const fA = (uint32_t*)(work + maxw);
  uint32_t* const fB = fA + capA;
  int32_t* const l_m12 = (int32_t*)(fB + capB);
  uint8_t* const l_dA = smem;
  uint8_t* const l_dB = smem + (size_t)capA * 32;

  if (tid < ORBX_TRIMATCH_MAX_LEVELS) {    // the level tables: constant indices into the kernel's arguments
    float s = 0.0f, q = 0.0f;
#pragma unroll
    for (int k = 0; k < ORBX_TRIMATCH_MAX_LEVELS; k++)
      if (tid == k) { s = g.scale[k]; q = g.sigma2[k]; }
    s_scale[tid] = s; s_sig[tid] = q;
  }

  for (int p = blockIdx.x; p < g.npairs; p += gridDim.x) {
    __syncthreads();                       // the previous pair's shared state has been read
    const int ia = g.pairs[2 * p], ib = g.pairs[2 * p + 1];
    int32_t* const o12 = g.m12 + (size_t)p * capA;
    bool ok = ia >= 0 && ia < g.a.nframes && ib >= 0 && ib < g.b.nframes;
    int nA = 0, nB = 0, kA = 0, kB = 0;
    if (ok) {
      nA = g.a.counts[2 * ia]; nB = g.b.counts[2 * ib]; kA = g.a.fv_n[ia]; kB = g.b.fv_n[ib];
      ok = nA >= 0 && nA <= capA && nB >= 0 && nB <= capB && kA >= 0 && kB >= 0;
    }
    if (!ok) { fail_row(g, p, o12); continue; }   // uniform over the workgroup
    kA = min(kA, capA); kB = min(kB, capB);
    const size_t oA = (size_t)ia * capA, oB = (size_t)ib * capB;
    const int32_t* const pA = g.a.fv_ptr + (size_t)ia * (capA + 1);
    const int32_t* const pB = g.b.fv_ptr + (size_t)ib * (capB + 1);
    const int totA = kA ? clampi(pA[kA], 0, capA) : 0, totB = kB ? clampi(pB[kB], 0, capB) : 0;
    const uint32_t* const gfA = g.a.fv_feat + oA;
    const uint32_t* const gfB = g.b.fv_feat + oB;
    const uint8_t* const kpA = g.a.kps + oA * sizeof(orbx_keypoint);
    const uint8_t* const kpB = g.b.kps + oB * sizeof(orbx_keypoint);
    const uint8_t* const hA = g.a.has_point ? g.a.has_point + oA : nullptr;
    const uint8_t* const hB = g.b.has_point ? g.b.has_point + oB : nullptr;
    const float* const uA = g.a.uright ? g.a.uright + oA : nullptr;
    const float* const uB = g.b.uright ? g.b.uright + oB : nullptr;
    // this instantiation's arrays: LDS or global, decided at compile time
    const uint8_t* const dA = LDS ? l_dA : g.a.desc + oA * 32;
    const uint8_t* const dB = LDS ? l_dB : g.b.desc + oB * 32;
    int32_t* const m12 = LDS ? l_m12 : o12;

    // ---- stage and check
    if (tid == 0) { s_cnt = 0; s_next = 0; s_bad = 0; s_nm = 0; }
    if (tid < 32) s_hist[tid] = 0;
    if (LDS) {
      stage_dma<kThreads>(l_dA, g.a.desc + oA * 32, nA * 2);
      stage_dma<kThreads>(l_dB, g.b.desc + oB * 32, nB * 2);
    }
    __syncthreads();                       // s_bad = 0 before anyone raises it
    for (int i = tid; i < totA; i += kThreads) {
      const uint32_t v = gfA[i];
      uint32_t e = kSkip;
      if (v >= (uint32_t)nA) s_bad = 1;
      else {
        const bool stereo = uA && uA[v] >= 0.0f;
        const bool skip = (hA && hA[v]) || (g.only_stereo && !stereo);
        e = v | (skip ? kSkip : 0u) | (stereo ? kStereo : 0u);
      }
      fA[i] = e;
    }
    for (int i = tid; i < totB; i += kThreads) {
      const uint32_t v = gfB[i];
      uint32_t e = kSkip;
      if (v >= (uint32_t)nB) s_bad = 1;
      else {
        if ((uint32_t)kp_field<int32_t>(kpB, v, kOctave) >= (uint32_t)g.nlevels) s_bad = 1;
        const bool stereo = uB && uB[v] >= 0.0f;
        const bool skip = (hB && hB[v]) || (g.only_stereo && !stereo);
        e = v | (skip ? kSkip : 0u) | (stereo ? kStereo : 0u);
      }
      fB[i] = e;
    }
    for (int i = tid; i < (LDS ? nA : capA); i += kThreads) m12[i] = -1;
    if (LDS) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the LDS-DMA loads have landed
    __syncthreads();
    if (s_bad) { fail_row(g, p, o12); continue; }

    // ---- the nodes both frames have, cut into chunks of queries
    common_nodes<kThreads>(g.a.fv_node + oA, pA, kA, totA, g.b.fv_node + oB, pB, kB, totB, [&](int a0, int a1, int b0, int b1) {
      const int nc = (a1 - a0 + kChunk - 1) / kChunk;
      const int k = atomicAdd(&s_cnt, nc);
      for (int c = 0; c < nc; c++)
        if (k + c < maxw) work[k + c] = make_int4(a0 + c * kChunk, min(a1, a0 + (c + 1) * kChunk), b0, b1);
    });
    __syncthreads();
    const int nwork = min(s_cnt, maxw);
    Geom G;
    {
      const float* const gp = g.geom + (size_t)p * 12;
      G.f00 = gp[0]; G.f01 = gp[1]; G.f02 = gp[2]; G.f10 = gp[3]; G.f11 = gp[4]; G.f12 = gp[5]; G.f20 = gp[6]; G.f21 = gp[7]; G.f22 = gp[8];
      G.epx = gp[9]; G.epy = gp[10];
    }

    // ---- one chunk of queries per wave at a time
    for (;;) {
      const int w = next_work(&s_next);
      if (w >= nwork) break;
      const int4 r = work[w];
      const int a0 = __builtin_amdgcn_readfirstlane(r.x), a1 = __builtin_amdgcn_readfirstlane(r.y);
      const int b0 = __builtin_amdgcn_readfirstlane(r.z), nb = __builtin_amdgcn_readfirstlane(r.w) - b0;
      const bool regs = nb <= 64;          // wave-uniform
      uint32_t my_e = kSkip;
      D8 my_db;
#pragma unroll
      for (int k = 0; k < 8; k++) my_db.w[k] = 0;
      if (regs && lane < nb) {
        my_e = fB[b0 + lane];
        my_db = load_desc(dB + (size_t)(my_e & kIdx) * 32);
      }
      for (int i = a0; i < a1; i++) {
        const uint32_t ea = (uint32_t)__builtin_amdgcn_readfirstlane((int)fA[i]);
        if (ea & kSkip) continue;
        const uint32_t fa = ea & kIdx;
        const bool mono1 = !(ea & kStereo);
        const D8 da = load_desc(dA + (size_t)fa * 32);   // wave-uniform address
        int key = INT_MAX;
        if (regs) {
          const int d = (my_e & kSkip) ? 256 : hamming(da, my_db);
          if (d <= kThLow) {
            const float x1 = kp_field<float>(kpA, fa, kX), y1 = kp_field<float>(kpA, fa, kY);
            if (gates(g, G, s_scale, s_sig, x1, y1, kpB, my_e & kIdx, mono1 && !(my_e & kStereo))) key = d << 16 | (0xFFFF - lane);
          }
        } else {
          for (int j = lane; j < nb; j += 64) {
            const uint32_t e = fB[b0 + j];
            if (e & kSkip) continue;
            const int d = hamming(da, load_desc(dB + (size_t)(e & kIdx) * 32));
            if (d <= kThLow) {
              const float x1 = kp_field<float>(kpA, fa, kX), y1 = kp_field<float>(kpA, fa, kY);
              if (gates(g, G, s_scale, s_sig, x1, y1, kpB, e & kIdx, mono1 && !(e & kStereo))) key = min(key, d << 16 | (0xFFFF - j));
            }
          }
        }
        const int m = wave_min(key);
        if (m != INT_MAX && lane == 0) m12[fa] = (int32_t)(fB[b0 + (0xFFFF - (m & 0xFFFF))] & kIdx);
      }
    }
    __syncthreads();

    // ---- the rotation filter and the output
    int i1 = -1, i2 = -1, i3 = -1;
    if (g.check_ori) {
      for (int q = tid; q < nA; q += kThreads) {
        const int v = m12[q];
        if (v >= 0) {
          const int bin = rot_bin(kp_field<float>(kpA, q, kAngle), kp_field<float>(kpB, v, kAngle));
          if (bin >= 0) atomicAdd(&s_hist[bin], 1);
        }
      }
      __syncthreads();
      if (tid == 0) three_maxima(s_hist, s_ind);
      __syncthreads();
      i1 = s_ind[0]; i2 = s_ind[1]; i3 = s_ind[2];
    }
    int cnt = 0;
    for (int q = tid; q < capA; q += kThreads) {
      int v = -1;
      if (q < nA) {
        v = m12[q];
        if (v >= 0 && g.check_ori) {
          const int bin = rot_bin(kp_field<float>(kpA, q, kAngle), kp_field<float>(kpB, v, kAngle));
          if (bin >= 0 && bin != i1 && bin != i2 && bin != i3) v = -1;
        }
        if (v < 0 || v >= nB) v = -1;
      }
      o12[q] = v;
      cnt += v >= 0;
    }
    if (cnt) atomicAdd(&s_nm, cnt);
    __syncthreads();
    if (tid == 0) g.nm[p] = s_nm;
  }
}

}  // namespace

struct orbx_trimatch : orbx::side::pair::PairHandle {};   // scratch: per workgroup the global path's work list and staged lists

namespace {

using namespace orbx::side;
using namespace orbx::side::pair;

Side to_side(const orbx_trimatch_side* s) {
  return {(const uint8_t*)s->d_kps, s->d_desc, s->d_counts, s->d_fv_node, s->d_fv_ptr, s->d_fv_feat, s->d_fv_n, s->d_has_point, s->d_uright,
          s->nframes, s->capacity};
}

// what both forms check before anything is copied or launched
int check_call(orbx_trimatch* m, const char* who, const orbx_trimatch_side* a, const orbx_trimatch_side* b, const void* pairs, int npairs,
               const void* geom, const float* scale, const float* sigma2, int nlevels, const void* m12, const void* nm) {
  int rc = check_sides<true>(m, who, a, b, ORBX_TRIMATCH_MAX_CAPACITY, "capacity above 65536", pairs && geom && m12 && nm,
                             "pairs, geom, matches12 or nmatches");
  if (rc != ORBX_OK) return rc;
  if (!scale || !sigma2) return fail(m, ORBX_E_INVALID, std::string(who) + "null scale_factor or level_sigma2");
  if (nlevels < 1 || nlevels > ORBX_TRIMATCH_MAX_LEVELS)
    return fail(m, ORBX_E_INVALID, std::string(who) + "nlevels = " + std::to_string(nlevels) + " (1 .. 16)");
  if ((rc = check_npairs(m, who, npairs)) != ORBX_OK) return rc;
  return check_sizes<true>(m, who, a, b, npairs, std::max(a->capacity, 12), "npairs * capacity");
}

}  // namespace

extern "C" {

int orbx_trimatch_create(orbx_trimatch** out, int device) {
  return create_handle(out, device, "orbx_trimatch_create", orbx_trimatch_destroy, [](orbx_trimatch* m) {
    return open_pair(m, "ORBX_TRIMATCH_LDS", nullptr, (const void*)k_tri_pairs<true>);
  });
}

void orbx_trimatch_destroy(orbx_trimatch* m) { destroy_handle(m); }

const char* orbx_trimatch_last_error(const orbx_trimatch* m) { return last_error(m); }

int orbx_trimatch_pairs_device(orbx_trimatch* m, const orbx_trimatch_side* a, const orbx_trimatch_side* b, const int32_t* d_pairs, int npairs,
                               const float* d_geom, const float* scale_factor, const float* level_sigma2, int nlevels, int only_stereo, int coarse,
                               int check_orientation, int32_t* d_matches12, int32_t* d_nmatches, void* stream) {
  if (!m) return ORBX_E_INVALID;
  const char* who = "orbx_trimatch_pairs_device: ";
  int rc = check_call(m, who, a, b, d_pairs, npairs, d_geom, scale_factor, level_sigma2, nlevels, d_matches12, d_nmatches);
  if (rc != ORBX_OK) return rc;
  rc = same_device(m, who, {a->d_kps, a->d_desc, a->d_fv_feat, a->d_has_point, a->d_uright, b->d_kps, b->d_desc, b->d_fv_feat, b->d_has_point,
                            b->d_uright, d_pairs, d_geom, d_matches12, d_nmatches}, "the handle");
  if (rc != ORBX_OK) return rc;
  ORBX_SIDE_HIP(m, hipSetDevice(m->device));
  const size_t capA = (size_t)a->capacity, capB = (size_t)b->capacity;
  const size_t lists = 16 * (size_t)max_work(a->capacity, b->capacity) + 4 * (capA + capB);
  const size_t lds = 32 * (capA + capB) + lists + 4 * capA;
  Args g;
  g.a = to_side(a); g.b = to_side(b);
  g.pairs = d_pairs; g.geom = d_geom; g.m12 = d_matches12; g.nm = d_nmatches;
  g.npairs = npairs; g.nlevels = nlevels; g.only_stereo = only_stereo != 0; g.coarse = coarse != 0; g.check_ori = check_orientation != 0;
  for (int l = 0; l < ORBX_TRIMATCH_MAX_LEVELS; l++) {
    g.scale[l] = l < nlevels ? scale_factor[l] : 0.0f;
    g.sigma2[l] = l < nlevels ? level_sigma2[l] : 0.0f;
  }
  return launch(m, lds <= (size_t)m->lds_limit, lds, (lists + 255) & ~(size_t)255, std::min(npairs, kMaxBlocks), kThreads, g, k_tri_pairs<true>,
                k_tri_pairs<false>, stream);
}

int orbx_trimatch_pairs(orbx_trimatch* m, const orbx_trimatch_side* a, const orbx_trimatch_side* b, const int32_t* pairs, int npairs,
                        const float* geom, const float* scale_factor, const float* level_sigma2, int nlevels, int only_stereo, int coarse,
                        int check_orientation, int32_t* matches12, int32_t* nmatches) {
  if (!m) return ORBX_E_INVALID;
  const char* who = "orbx_trimatch_pairs: ";
  int rc = check_call(m, who, a, b, pairs, npairs, geom, scale_factor, level_sigma2, nlevels, matches12, nmatches);
  if (rc != ORBX_OK) return rc;
  const auto arrays = side_arrays<true, orbx_trimatch_side>({{offsetof(orbx_trimatch_side, d_has_point), 0, 1, true},
                                                             {offsetof(orbx_trimatch_side, d_uright), 0, 4, true}});
  Stager io;
  const StagedSides off = stage_sides(io, a, b, arrays);
  const size_t o_pairs = io.in(pairs, (size_t)npairs * 8), o_geom = io.in(geom, (size_t)npairs * 12 * 4);
  const size_t o_12 = io.out(matches12, (size_t)npairs * a->capacity * 4), o_nm = io.out(nmatches, (size_t)npairs * 4);
  if ((rc = upload(m, io)) != ORBX_OK) return rc;
  uint8_t* d = m->io.p;
  orbx_trimatch_side ds[2];
  device_sides(d, off, a, b, arrays, ds);
  rc = orbx_trimatch_pairs_device(m, &ds[0], &ds[1], (const int32_t*)(d + o_pairs), npairs, (const float*)(d + o_geom), scale_factor, level_sigma2,
                                  nlevels, only_stereo, coarse, check_orientation, (int32_t*)(d + o_12), (int32_t*)(d + o_nm), m->st);
  if (rc != ORBX_OK) return rc;
  return download(m, io);
}

}  // extern "C"
