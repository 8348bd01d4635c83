// The batched stereo front-end (include/orbx_stereo.h): Frame::ComputeStereoMatches (src/Frame.cc:811-981) for B rectified pairs on the
// pyramids two product contexts left resident by their last batch extraction, and both extractions + the association in one call.
//
// Per frame the arithmetic is k_stereo_match / k_stereo_filter's (csrc/orbx_search.hip), which restate the reference literally: the same
// gates, the first minimum of the Hamming distance in ascending right index, the 11 x 11 SAD over 11 shifts on the left keypoint's level,
// the parabola, the `disparity <= 0` branch and the median filter, every float operation a separate IEEE op (-ffp-contract=off, __f*_rn).
// What changes is the shape of the work for a batch:
//   k_sb_gates   one 8-byte word per right keypoint: x (float bits) | octave, row band ceil / floor(y +- 2 scale[octave]) clamped to [-1, 4096]
//                (rows are < 4096, so the clamp keeps every comparison with a row in [0, 4095])
//   k_sb_match   16 left keypoints of ONE frame per workgroup, 4 per wave tested together: the frame's right gates are staged in LDS once per
//                workgroup (tiles of kSbTile), every lane tests one right keypoint against the wave's 4 left keypoints, and only a right
//                keypoint that passes some gate has its descriptor read.  Then the SAD window per accepted left keypoint, as k_stereo_match.
//   k_sb_filter  one workgroup per frame: the (n/2)-th smallest SAD by rank counting, LDS when the frame's SADs fit, global memory otherwise.
// The library reads the buffers of a product context (orbx_internal.h) the way liborbx_debug.so does and changes none of them.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../orbx_internal.h"
#include "../side/orbx_handle.h"
#include "../side/orbx_rig.h"
#include "../../../include/orbx_stereo.h"

namespace {

using orbx::kMaxLevels;

constexpr int kSbWaves = 4, kSbPerWave = 4, kSbPerGroup = kSbWaves * kSbPerWave;
constexpr int kSbTile = 2048;        // right gates per LDS tile: 16 KiB (the tile a call uses: 1 .. kSbTile, ORBX_STEREO_TILE)
constexpr int kSbLdsSad = 12288;     // SADs of one frame the filter keeps in LDS: 48 KiB (frames above 0 .. kSbLdsSad SADs, ORBX_STEREO_FILTER_LDS, read
                                     // them from global memory)

struct SbSide {
  const uint8_t* lv0;                // level 0 of frame 0 (the caller's frames, or the context's realigned copy)
  long long lv0_row, lv0_frame;      // its strides
  const uint8_t* pyr;                // d_pyr: levels >= 1 of frame f at pyr + f * pyr_bytes + off[l]
  long long pyr_bytes;
  long long off[kMaxLevels];
  int pitch[kMaxLevels];
};
struct SbGeom {
  SbSide L, R;
  int w[kMaxLevels], h0;
  float scale[kMaxLevels], inv_scale[kMaxLevels];
};

__device__ inline const uint8_t* sb_plane(const SbSide& s, int f, int l, int* pitch) {
  if (l == 0) { *pitch = (int)s.lv0_row; return s.lv0 + (size_t)f * (size_t)s.lv0_frame; }
  *pitch = s.pitch[l];
  return s.pyr + (size_t)f * (size_t)s.pyr_bytes + (size_t)s.off[l];
}

__device__ inline int sb_clamp_row(int r) { return r < -1 ? -1 : (r > 4096 ? 4096 : r); }

// gates[f][i] = {x bits, octave | (minr + 1) << 4 | (maxr + 1) << 17} for i < nR; a frame with a negative count has no gates
__global__ __launch_bounds__(256) void k_sb_gates(SbGeom g, const orbx_keypoint* __restrict__ kpsR, const int32_t* __restrict__ countsR, int cap,
                                                  uint2* __restrict__ gates) {
  const int f = blockIdx.y;
  const int nR = min(countsR[2 * f], cap);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < nR; i += gridDim.x * 256) {
    const orbx_keypoint kpR = kpsR[(size_t)f * cap + i];
    const float r = __fmul_rn(2.0f, g.scale[kpR.octave]);
    const int maxr = (int)ceilf(__fadd_rn(kpR.y, r)), minr = (int)floorf(__fsub_rn(kpR.y, r));
    gates[(size_t)f * cap + i] = make_uint2(__float_as_uint(kpR.x), (uint32_t)kpR.octave | (uint32_t)(sb_clamp_row(minr) + 1) << 4 |
                                                                        (uint32_t)(sb_clamp_row(maxr) + 1) << 17);
  }
}

// grid (ceil(cap / 16), nframes).  Writes u_right / depth / sad of every slot of its 16 (-1 past the frame's left count).
__global__ __launch_bounds__(256) void k_sb_match(SbGeom g, const orbx_keypoint* __restrict__ kpsL, const uint8_t* __restrict__ descL,
                                                  const int32_t* __restrict__ countsL, const uint8_t* __restrict__ descR,
                                                  const int32_t* __restrict__ countsR, const uint2* __restrict__ gates, int cap, int tile,
                                                  float mb, float mbf, float* __restrict__ uRight, float* __restrict__ depth, int32_t* __restrict__ sad) {
  __shared__ uint2 s_gate[kSbTile];
  __shared__ int s_part[kSbWaves][128];
  __shared__ unsigned long long s_best[kSbWaves][kSbPerWave];
  const int f = blockIdx.y;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int cL = countsL[2 * f], cR = countsR[2 * f];
  const bool bad = cL < 0 || cR < 0;
  const int nL = bad ? 0 : min(cL, cap), nR = bad ? 0 : min(cR, cap);
  const int i0 = blockIdx.x * kSbPerGroup + wv * kSbPerWave;   // this wave's first left slot
  const size_t fo = (size_t)f * cap;
  const float minD = 0.0f, maxD = __fdiv_rn(mbf, mb);
  // the wave's 4 left keypoints (wave-uniform)
  bool act[kSbPerWave];
  int row[kSbPerWave], lev[kSbPerWave];
  float minU[kSbPerWave], maxU[kSbPerWave];
  uint4 qa[kSbPerWave], qb[kSbPerWave];
  unsigned long long best[kSbPerWave];
#pragma unroll
  for (int k = 0; k < kSbPerWave; k++) {
    const int iL = i0 + k;
    act[k] = false; row[k] = 0; lev[k] = 0; minU[k] = 0.0f; maxU[k] = 0.0f; best[k] = ~0ull;
    qa[k] = make_uint4(0, 0, 0, 0); qb[k] = qa[k];
    if (iL < nL && nR > 0) {
      const orbx_keypoint kpL = kpsL[fo + iL];
      lev[k] = kpL.octave;
      row[k] = (int)kpL.y;
      minU[k] = __fsub_rn(kpL.x, maxD); maxU[k] = __fsub_rn(kpL.x, minD);
      act[k] = row[k] >= 0 && row[k] < g.h0 && !(maxU[k] < 0);
      if (act[k]) {
        const uint4* qp = (const uint4*)(descL + (fo + iL) * 32);
        qa[k] = qp[0]; qb[k] = qp[1];
      }
    }
  }
  // (1) gates from LDS, descriptors only behind a passed gate; nR is uniform over the workgroup, so are the tile loop and its barriers
  for (int t0 = 0; t0 < nR; t0 += tile) {
    const int tn = min(tile, nR - t0);
    __syncthreads();
    for (int i = threadIdx.x; i < tn; i += 256) s_gate[i] = gates[fo + t0 + i];
    __syncthreads();
    for (int j = lane; j < tn; j += 64) {
      const uint2 gw = s_gate[j];
      const float x = __uint_as_float(gw.x);
      const int oct = (int)(gw.y & 15u), minr = (int)((gw.y >> 4) & 0x1fffu) - 1, maxr = (int)(gw.y >> 17) - 1;
      bool pass[kSbPerWave];
      bool any = false;
#pragma unroll
      for (int k = 0; k < kSbPerWave; k++) {
        pass[k] = act[k] && !(row[k] < minr || row[k] > maxr) && !(oct < lev[k] - 1 || oct > lev[k] + 1) && x >= minU[k] && x <= maxU[k];
        any |= pass[k];
      }
      if (!any) continue;
      const int iR = t0 + j;
      const uint4* tp = (const uint4*)(descR + (fo + iR) * 32);
      const uint4 ta = tp[0], tb = tp[1];
#pragma unroll
      for (int k = 0; k < kSbPerWave; k++) {
        if (!pass[k]) continue;
        const int d = __popc(qa[k].x ^ ta.x) + __popc(qa[k].y ^ ta.y) + __popc(qa[k].z ^ ta.z) + __popc(qa[k].w ^ ta.w) +
                      __popc(qb[k].x ^ tb.x) + __popc(qb[k].y ^ tb.y) + __popc(qb[k].z ^ tb.z) + __popc(qb[k].w ^ tb.w);
        const unsigned long long key = ((unsigned long long)d << 32) | (uint32_t)iR;
        best[k] = key < best[k] ? key : best[k];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kSbPerWave; k++) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long p = __shfl_xor(best[k], o); best[k] = p < best[k] ? p : best[k]; }
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kSbPerWave; k++) s_best[wv][k] = best[k];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  // (2) + (3) per left keypoint of the wave, as k_stereo_match
  for (int k = 0; k < kSbPerWave; k++) {
    const int iL = i0 + k;
    if (iL >= cap) break;
    float out_u = -1.0f, out_d = -1.0f;
    int out_sad = -1;
    const unsigned long long bk = s_best[wv][k];
    const int bestDist = bk == ~0ull ? 256 : (int)(bk >> 32);
    const int TH_HIGH = 100, thOrbDist = 75;
    if (iL < nL && bestDist < TH_HIGH && bestDist < thOrbDist) {   // wave-uniform
      const orbx_keypoint kpL = kpsL[fo + iL];
      const int levelL = kpL.octave;
      const float uL = kpL.x;
      const int bestIdxR = (int)(uint32_t)bk;
      const float uR0 = __uint_as_float(gates[fo + bestIdxR].x);
      const float scaleFactor = g.inv_scale[levelL];
      const float scaleduL = roundf(__fmul_rn(kpL.x, scaleFactor));
      const float scaledvL = roundf(__fmul_rn(kpL.y, scaleFactor));
      const float scaleduR0 = roundf(__fmul_rn(uR0, scaleFactor));
      const int wnd = 5, Ls = 5;
      const float iniu = __fsub_rn(__fadd_rn(scaleduR0, (float)Ls), (float)wnd);
      const float endu = __fadd_rn(__fadd_rn(__fadd_rn(scaleduR0, (float)Ls), (float)wnd), 1.0f);
      if (!(iniu < 0 || endu >= (float)g.w[levelL])) {
        const int r0 = (int)__fsub_rn(scaledvL, (float)wnd), cL0 = (int)__fsub_rn(scaleduL, (float)wnd);
        int pL, pR;
        const uint8_t* IL = sb_plane(g.L, f, levelL, &pL);
        const uint8_t* IR = sb_plane(g.R, f, levelL, &pR);
        for (int it = lane; it < 121; it += 64) {
          const int si = it / 11, rr = it - si * 11;
          const int cR0 = (int)__fsub_rn(__fadd_rn(scaleduR0, (float)(si - Ls)), (float)wnd);
          const uint8_t* a = IL + (size_t)(r0 + rr) * pL + cL0;
          const uint8_t* b = IR + (size_t)(r0 + rr) * pR + cR0;
          int acc = 0;
#pragma unroll
          for (int cc = 0; cc < 11; cc++) { const int d = (int)a[cc] - (int)b[cc]; acc += d < 0 ? -d : d; }
          s_part[wv][it] = acc;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (lane == 0) {
          float vDists[11];
          int bestS = 0x7fffffff, bestincR = 0;
#pragma unroll
          for (int si = 0; si < 11; si++) {
            int acc = 0;
            for (int rr = 0; rr < 11; rr++) acc += s_part[wv][si * 11 + rr];
            const float dist = (float)acc;
            if (dist < (float)bestS) { bestS = acc; bestincR = si - Ls; }
            vDists[si] = dist;
          }
          if (!(bestincR == -Ls || bestincR == Ls)) {
            // vDists[Ls + bestincR + {-1, 0, 1}] without a dynamic index into the array (no scratch): a select over the 11 entries
            float dist1 = 0.0f, dist2 = 0.0f, dist3 = 0.0f;
#pragma unroll
            for (int si = 0; si < 11; si++) {
              if (si == Ls + bestincR - 1) dist1 = vDists[si];
              if (si == Ls + bestincR) dist2 = vDists[si];
              if (si == Ls + bestincR + 1) dist3 = vDists[si];
            }
            const float den = __fmul_rn(2.0f, __fsub_rn(__fadd_rn(dist1, dist3), __fmul_rn(2.0f, dist2)));
            const float deltaR = __fdiv_rn(__fsub_rn(dist1, dist3), den);
            if (!(deltaR < -1 || deltaR > 1)) {
              float bestuR = __fmul_rn(g.scale[levelL], __fadd_rn(__fadd_rn(scaleduR0, (float)bestincR), deltaR));
              float disparity = __fsub_rn(uL, bestuR);
              if (disparity >= minD && disparity < maxD) {
                if (disparity <= 0) { disparity = (float)0.01; bestuR = (float)__dsub_rn((double)uL, 0.01); }
                out_d = __fdiv_rn(mbf, disparity);
                out_u = bestuR;
                out_sad = bestS;
              }
            }
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // s_part is reused by the wave's next keypoint
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      }
    }
    if (lane == 0) { uRight[fo + iL] = out_u; depth[fo + iL] = out_d; sad[fo + iL] = out_sad; }
  }
}

// The rank count and the filter of one frame over its N SADs, read through `sadAt` (LDS or global memory: one instantiation each, so that
// the LDS path compiles to ds_read and not to flat loads through a pointer the compiler cannot place)
template <typename SadAt>
__device__ __forceinline__ int sb_rank_filter(int N, int t, SadAt sadAt, float* __restrict__ U, float* __restrict__ D, int& s_n, int& s_median,
                                              int& s_kept) {
  int mine = 0;
  for (int i = t; i < N; i += 1024) mine += sadAt(i) >= 0;
  if (mine) atomicAdd(&s_n, mine);
  __syncthreads();
  const int n = s_n;
  if (n > 0) {   // block-uniform
    const int k = n / 2;
    for (int i = t; i < N; i += 1024) {
      const int v = sadAt(i);
      if (v < 0) continue;
      int lo = 0, eq = 0;
      for (int j = 0; j < N; j++) { const int u = sadAt(j); lo += (u >= 0 && u < v); eq += (u == v); }
      if (lo <= k && k < lo + eq) s_median = v;   // every thread that hits writes the same value
    }
    __syncthreads();
    const float thDist = __fmul_rn(1.5f * 1.4f, (float)s_median);
    int kept = 0;
    for (int i = t; i < N; i += 1024) {
      const int v = sadAt(i);
      if (v < 0) continue;
      if ((float)v < thDist) kept++;
      else { U[i] = -1.0f; D[i] = -1.0f; }
    }
    if (kept) atomicAdd(&s_kept, kept);
  }
  __syncthreads();
  return s_kept;
}

// One workgroup per frame: the median filter of src/Frame.cc:969-981 as k_stereo_filter (only the (n/2)-th smallest SAD matters: rank
// counting, no sort).  kept[f] = -1 for a frame with a negative count (its slots are all -1 already).
__global__ __launch_bounds__(1024) void k_sb_filter(const int32_t* __restrict__ countsL, const int32_t* __restrict__ countsR, int cap, int lds_cap,
                                                    float* __restrict__ uRight, float* __restrict__ depth, const int32_t* __restrict__ sad,
                                                    int32_t* __restrict__ kept_out) {
  __shared__ int s_n, s_median, s_kept;
  __shared__ int32_t s_sad[kSbLdsSad];
  const int f = blockIdx.x, t = threadIdx.x;
  const int cL = countsL[2 * f], cR = countsR[2 * f];
  if (cL < 0 || cR < 0) {   // block-uniform
    if (t == 0) kept_out[f] = -1;
    return;
  }
  const int N = min(cL, cap);
  const size_t fo = (size_t)f * cap;
  const int32_t* G = sad + fo;
  if (t == 0) { s_n = 0; s_median = -1; s_kept = 0; }
  const bool lds = N <= lds_cap;   // block-uniform
  if (lds) for (int i = t; i < N; i += 1024) s_sad[i] = G[i];
  __syncthreads();
  const int kept = lds ? sb_rank_filter(N, t, [&](int i) { return s_sad[i]; }, uRight + fo, depth + fo, s_n, s_median, s_kept)
                       : sb_rank_filter(N, t, [&](int i) { return G[i]; }, uRight + fo, depth + fo, s_n, s_median, s_kept);
  if (t == 0) kept_out[f] = kept;
}

}  // namespace

struct orbx_stereo : orbx::side::Handle {   // scratch: gates [frames][cap] + SADs [frames][cap]; io: keypoints, descriptors, counts and results
  orbx_ctx* left = nullptr;                 // (never frames: level 0 of a batch must live in memory its context owns, as it outlives the handle)
  orbx_ctx* right = nullptr;
  float mb = 0.0f, mbf = 0.0f;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  int tile = kSbTile, filter_lds = kSbLdsSad;     // ORBX_STEREO_TILE / ORBX_STEREO_FILTER_LDS at create (the tiled and the global-memory paths)
};

namespace {

using namespace orbx::side;

const char* param_mismatch(const orbx_ctx* a, const orbx_ctx* b) { return rig_mismatch(a, b); }

void side_geom(const orbx_ctx* c, SbSide* s) {
  s->lv0 = c->last_imgs; s->lv0_row = (long long)c->last_row_stride; s->lv0_frame = (long long)c->last_frame_stride;
  s->pyr = c->d_pyr; s->pyr_bytes = (long long)c->geo.pyr_bytes;
  for (int l = 0; l < c->nlevels; l++) {
    s->off[l] = l == 0 ? 0 : (long long)c->geo.lv[l].plane_off;
    s->pitch[l] = l == 0 ? (int)c->last_row_stride : c->geo.lv[l].pitch;
  }
}

}  // namespace

extern "C" {

int orbx_stereo_create(orbx_stereo** out, orbx_ctx* left, orbx_ctx* right, float mb, float mbf) {
  if (out) *out = nullptr;
  auto bad = [](const char* m, int code = ORBX_E_INVALID) { return create_fail(code, "orbx_stereo_create", m); };
  if (!out || !left || !right) return bad("null argument");
  if (left == right) return bad("the left and the right side need two contexts");
  if (const char* m = param_mismatch(left, right)) return bad(m);
  if (!(mb > 0)) return bad("mb (the baseline) must be > 0");
  if (!std::isfinite(mbf)) return bad("mbf must be finite");
  orbx_stereo* s = new orbx_stereo();
  s->left = left; s->right = right; s->mb = mb; s->mbf = mbf;
  if (const char* e = std::getenv("ORBX_STEREO_TILE")) s->tile = std::max(1, std::min(kSbTile, std::atoi(e)));
  if (const char* e = std::getenv("ORBX_STEREO_FILTER_LDS")) s->filter_lds = std::max(0, std::min(kSbLdsSad, std::atoi(e)));
  const char* e = open_handle(s, left->device);
  if (!e && (hipEventCreateWithFlags(&s->ev_fork, hipEventDisableTiming) != hipSuccess ||
             hipEventCreateWithFlags(&s->ev_join, hipEventDisableTiming) != hipSuccess)) {
    (void)hipGetLastError();
    e = "stream / event creation failed";
  }
  if (e) { orbx_stereo_destroy(s); return bad(e, ORBX_E_DEVICE); }
  *out = s;
  return ORBX_OK;
}

void orbx_stereo_destroy(orbx_stereo* s) {
  if (!s) return;
  close_handle(s);
  if (s->ev_fork) (void)hipEventDestroy(s->ev_fork);
  if (s->ev_join) (void)hipEventDestroy(s->ev_join);
  delete s;
}

const char* orbx_stereo_last_error(const orbx_stereo* s) { return last_error(s); }

int orbx_stereo_match_batch_device(orbx_stereo* s, int nframes, const orbx_keypoint* d_kpsL, const uint8_t* d_descL, const int32_t* d_countsL,
                                   const orbx_keypoint* d_kpsR, const uint8_t* d_descR, const int32_t* d_countsR, float* d_u_right, float* d_depth,
                                   int32_t* d_kept, void* stream) {
  if (!s) return ORBX_E_INVALID;
  const orbx_ctx* L = s->left;
  const orbx_ctx* R = s->right;
  if (!d_kpsL || !d_descL || !d_countsL || !d_kpsR || !d_descR || !d_countsR || !d_u_right || !d_depth || !d_kept)
    return fail(s, ORBX_E_INVALID, "orbx_stereo_match_batch_device: null buffer");
  if (const char* m = param_mismatch(L, R)) return fail(s, ORBX_E_INVALID, std::string("orbx_stereo_match_batch_device: ") + m);
  if (nframes < 1 || nframes > L->last_nframes || nframes > R->last_nframes)
    return fail(s, ORBX_E_INVALID, "orbx_stereo_match_batch_device: nframes = " + std::to_string(nframes) + " is outside [1, " +
                                       std::to_string(std::min(L->last_nframes, R->last_nframes)) + "], the frames both last batches hold");
  if (!L->d_geo || !R->d_geo || !L->last_imgs || !R->last_imgs || L->geo.rows != R->geo.rows || L->geo.cols != R->geo.cols)
    return fail(s, ORBX_E_INVALID, "orbx_stereo_match_batch_device: the two last batches have different shapes");
  const int cap = L->out_cap;
  ORBX_SIDE_HIP(s, hipSetDevice(s->device));
  const size_t slots = (size_t)nframes * cap;
  orbx::BlobLayout sc;
  const size_t o_gates = sc.add(slots * sizeof(uint2)), o_sad = sc.add(slots * sizeof(int32_t));
  int rc = grow(s, &s->scratch, sc.size);
  if (rc != ORBX_OK) return rc;
  uint2* d_gates = (uint2*)(s->scratch.p + o_gates);
  int32_t* d_sad = (int32_t*)(s->scratch.p + o_sad);
  hipStream_t st = stream ? (hipStream_t)stream : L->stream;
  if ((rc = wait_previous(s, st)) != ORBX_OK) return rc;
  SbGeom g;
  std::memset(&g, 0, sizeof(g));
  side_geom(L, &g.L);
  side_geom(R, &g.R);
  g.h0 = L->geo.lv[0].h;
  for (int l = 0; l < L->nlevels; l++) { g.w[l] = L->geo.lv[l].w; g.scale[l] = L->scale[l]; g.inv_scale[l] = L->inv_scale[l]; }
  hipLaunchKernelGGL(k_sb_gates, dim3((unsigned)((cap + 255) / 256), (unsigned)nframes), dim3(256), 0, st, g, d_kpsR, d_countsR, cap, d_gates);
  hipLaunchKernelGGL(k_sb_match, dim3((unsigned)((cap + kSbPerGroup - 1) / kSbPerGroup), (unsigned)nframes), dim3(256), 0, st, g, d_kpsL, d_descL,
                     d_countsL, d_descR, d_countsR, (const uint2*)d_gates, cap, s->tile, s->mb, s->mbf, d_u_right, d_depth, d_sad);
  hipLaunchKernelGGL(k_sb_filter, dim3((unsigned)nframes), dim3(1024), 0, st, d_countsL, d_countsR, cap, s->filter_lds, d_u_right, d_depth,
                     (const int32_t*)d_sad, d_kept);
  return record_call(s, st);
}

int orbx_stereo_extract_batch_device(orbx_stereo* s, const uint8_t* d_imgsL, const uint8_t* d_imgsR, int nframes, int rows, int cols,
                                     size_t row_stride, size_t frame_stride, orbx_keypoint* d_kpsL, uint8_t* d_descL, int32_t* d_countsL,
                                     orbx_keypoint* d_kpsR, uint8_t* d_descR, int32_t* d_countsR, float* d_u_right, float* d_depth,
                                     int32_t* d_kept, void* stream) {
  if (!s) return ORBX_E_INVALID;
  if (!d_imgsL || !d_imgsR || nframes < 1) return fail(s, ORBX_E_INVALID, "orbx_stereo_extract_batch_device: no frames");
  if (const char* m = param_mismatch(s->left, s->right)) return fail(s, ORBX_E_INVALID, std::string("orbx_stereo_extract_batch_device: ") + m);
  ORBX_SIDE_HIP(s, hipSetDevice(s->device));
  hipStream_t st = stream ? (hipStream_t)stream : s->left->stream;
  // the right side on the right context's own stream (a NULL stream argument), forked from and joined back into the caller's: the context
  // then remembers no stream of this handle, which may be destroyed before the context
  hipStream_t sr = s->right->stream;
  ORBX_SIDE_HIP(s, hipEventRecord(s->ev_fork, st));
  ORBX_SIDE_HIP(s, hipStreamWaitEvent(sr, s->ev_fork, 0));
  int rc = orbx_extract_batch_device(s->left, d_imgsL, nframes, rows, cols, row_stride, frame_stride, 0, 0, d_kpsL, d_descL, d_countsL, st);
  if (rc != ORBX_OK) return fail(s, rc, std::string("left extraction: ") + orbx_last_error(s->left));
  rc = orbx_extract_batch_device(s->right, d_imgsR, nframes, rows, cols, row_stride, frame_stride, 0, 0, d_kpsR, d_descR, d_countsR, nullptr);
  const hipError_t e1 = hipEventRecord(s->ev_join, sr), e2 = hipStreamWaitEvent(st, s->ev_join, 0);   // joined whether or not it succeeded
  if (rc != ORBX_OK) return fail(s, rc, std::string("right extraction: ") + orbx_last_error(s->right));
  ORBX_SIDE_HIP(s, e1);
  ORBX_SIDE_HIP(s, e2);
  return orbx_stereo_match_batch_device(s, nframes, d_kpsL, d_descL, d_countsL, d_kpsR, d_descR, d_countsR, d_u_right, d_depth, d_kept, st);
}

int orbx_stereo_extract_batch(orbx_stereo* s, const uint8_t* imgsL, const uint8_t* imgsR, int nframes, int rows, int cols, size_t row_stride,
                              size_t frame_stride, orbx_keypoint* kpsL, uint8_t* descL, int32_t* countsL, orbx_keypoint* kpsR, uint8_t* descR,
                              int32_t* countsR, float* u_right, float* depth, int32_t* kept) {
  if (!s) return ORBX_E_INVALID;
  if (!imgsL || !imgsR || nframes < 1 || rows < 1 || cols < 1) return fail(s, ORBX_E_INVALID, "orbx_stereo_extract_batch: no frames");
  if (!kpsL || !descL || !countsL || !kpsR || !descR || !countsR || !u_right || !depth || !kept)
    return fail(s, ORBX_E_INVALID, "orbx_stereo_extract_batch: bad arguments");
  if (const char* m = param_mismatch(s->left, s->right)) return fail(s, ORBX_E_INVALID, std::string("orbx_stereo_extract_batch: ") + m);
  // each side through the product's own host-buffer batch: it stages the frames in memory its context owns (level 0 of the batch, which the
  // context's later calls read — after this handle may be gone) and returns keypoints, descriptors and counts in the caller's buffers
  int rc = orbx_extract_batch(s->left, imgsL, nframes, rows, cols, row_stride, frame_stride, 0, 0, kpsL, descL, countsL);
  if (rc != ORBX_OK) return fail(s, rc, std::string("left extraction: ") + orbx_last_error(s->left));
  rc = orbx_extract_batch(s->right, imgsR, nframes, rows, cols, row_stride, frame_stride, 0, 0, kpsR, descR, countsR);
  if (rc != ORBX_OK) return fail(s, rc, std::string("right extraction: ") + orbx_last_error(s->right));
  const int cap = s->left->out_cap;
  const size_t nk = (size_t)nframes * cap;
  orbx::BlobLayout io;
  const size_t o_kL = io.add(nk * sizeof(orbx_keypoint)), o_kR = io.add(nk * sizeof(orbx_keypoint)), o_dL = io.add(nk * 32),
               o_dR = io.add(nk * 32), o_cL = io.add((size_t)nframes * 8), o_cR = io.add((size_t)nframes * 8), o_u = io.add(nk * 4),
               o_d = io.add(nk * 4), o_k = io.add((size_t)nframes * 4);
  ORBX_SIDE_HIP(s, hipSetDevice(s->device));
  hipStream_t st = s->st;
  if ((rc = grow(s, &s->io, io.size)) != ORBX_OK) return rc;
  uint8_t* d = s->io.p;
  ORBX_SIDE_HIP(s, hipMemcpyAsync(d + o_kL, kpsL, nk * sizeof(orbx_keypoint), hipMemcpyHostToDevice, st));
  ORBX_SIDE_HIP(s, hipMemcpyAsync(d + o_kR, kpsR, nk * sizeof(orbx_keypoint), hipMemcpyHostToDevice, st));
  ORBX_SIDE_HIP(s, hipMemcpyAsync(d + o_dL, descL, nk * 32, hipMemcpyHostToDevice, st));
  ORBX_SIDE_HIP(s, hipMemcpyAsync(d + o_dR, descR, nk * 32, hipMemcpyHostToDevice, st));
  ORBX_SIDE_HIP(s, hipMemcpyAsync(d + o_cL, countsL, (size_t)nframes * 8, hipMemcpyHostToDevice, st));
  ORBX_SIDE_HIP(s, hipMemcpyAsync(d + o_cR, countsR, (size_t)nframes * 8, hipMemcpyHostToDevice, st));
  rc = orbx_stereo_match_batch_device(s, nframes, (const orbx_keypoint*)(d + o_kL), d + o_dL, (const int32_t*)(d + o_cL),
                                      (const orbx_keypoint*)(d + o_kR), d + o_dR, (const int32_t*)(d + o_cR), (float*)(d + o_u), (float*)(d + o_d),
                                      (int32_t*)(d + o_k), st);
  if (rc != ORBX_OK) return rc;
  ORBX_SIDE_HIP(s, hipMemcpyAsync(u_right, d + o_u, nk * 4, hipMemcpyDeviceToHost, st));
  ORBX_SIDE_HIP(s, hipMemcpyAsync(depth, d + o_d, nk * 4, hipMemcpyDeviceToHost, st));
  ORBX_SIDE_HIP(s, hipMemcpyAsync(kept, d + o_k, (size_t)nframes * 4, hipMemcpyDeviceToHost, st));
  return finish_host(s);
}

}  // extern "C"
