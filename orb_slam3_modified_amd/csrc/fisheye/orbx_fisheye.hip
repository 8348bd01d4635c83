// The batched two-camera rig front-end (include/orbx_fisheye.h): Frame::ComputeStereoFishEyeMatches (src/Frame.cc:1126-1166) for B fisheye
// pairs on the descriptors two batch extractions left in HBM.  The sizes of the B problems exist only on the device (d_counts), so every
// launch covers the whole batch and every workgroup finds its frame's ranges itself:
//   k_fe_knn      grid (ceil(capL / 256), nframes): a lane owns ONE query -- left row blockIdx.x * 256 + threadIdx.x, its 256 bits in 8
//                 VGPRs -- and the workgroup streams the frame's train rows through LDS in tiles its 256 queries share.  Per pair 8 xor +
//                 8 accumulating popcounts and the three-instruction top-2 update on (distance << 22 | right row) keys, which orders ties as a
//                 sequential scan does.  The ratio test of :1151 runs here; a wave's 64 verdicts leave as one ballot word.
//   k_fe_compact  one workgroup per frame: a prefix sum over the ballot words' popcounts places every accepted pair, so the list ascends in
//                 the left row whatever the order the workgroups of k_fe_knn ran in; d_npairs and the {-1, -1} tail.
//   k_fe_finish   one workgroup per frame: :1134-1137 and :1157-1163.  The pairs ascend in `left`, so "the last pair that names a right row
//                 stays" is one integer atomic max.
// Why LDS tiles and not wave-uniform scalar operands (k_knn2_partial's form): here a workgroup's four waves walk the SAME train rows, so a
// tile is fetched from memory once per workgroup with coalesced 16-byte loads and read back as broadcast ds_read_b128 (every lane the same
// address: no bank conflict), where the scalar form issues the row's loads once per wave and waits for each at the head of a short loop; a
// frame's 300 .. 600 train rows are one or two tiles.  The tile is also the only size edge of the kernel, and ORBX_FISHEYE_TILE moves it.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../side/orbx_handle.h"
#include "../side/orbx_pair_device.h"
#include "../side/orbx_rig.h"
#include "../../../include/orbx_fisheye.h"

namespace {

using namespace orbx::side::dev;

constexpr int kFeQueries = 256;      // queries (lanes) per workgroup
constexpr int kFeTile = 512;         // train rows per LDS tile: 16 KiB (the tile a call uses: 1 .. kFeTile, ORBX_FISHEYE_TILE)
constexpr int kFeMaxCap = 1 << kKeyIndexBits;
constexpr int kFeEmpty = -1, kFeMalformed = -2;

struct FeFrame { int status, q0, q1, t0, t1; };   // status 0: queries [q0, q1) of the left rows, train rows [t0, t1) of the right rows

// the frame's ranges, checked before anything is addressed with them
__device__ __forceinline__ FeFrame fe_frame(const int32_t* __restrict__ countsL, const int32_t* __restrict__ countsR, int f, int capL, int capR) {
  const int nL = countsL[2 * f], mL = countsL[2 * f + 1], nR = countsR[2 * f], mR = countsR[2 * f + 1];
  FeFrame r{0, 0, 0, 0, 0};
  if (nL == -1 || nR == -1) r.status = kFeEmpty;
  else if (nL < 0 || nL > capL || mL < 0 || mL > nL || nR < 0 || nR > capR || mR < 0 || mR > nR) r.status = kFeMalformed;
  else { r.q0 = mL; r.q1 = nL; r.t0 = mR; r.t1 = nR; }
  return r;
}

// (*it)[0].distance < (*it)[1].distance * 0.7 (:1151): DMatch::distance is a float, the literal a double
__device__ __forceinline__ bool fe_ratio(int d0, int d1) { return (double)(float)d0 < __dmul_rn((double)(float)d1, 0.7); }

// words: [nframes][ceil(capL / 64)] ballots of the accepted rows
__global__ __launch_bounds__(kFeQueries) void k_fe_knn(const uint8_t* __restrict__ descL, const int32_t* __restrict__ countsL,
                                                       const uint8_t* __restrict__ descR, const int32_t* __restrict__ countsR, int capL, int capR,
                                                       int tile, int32_t* __restrict__ knn_idx, int32_t* __restrict__ knn_dist,
                                                       unsigned long long* __restrict__ words) {
  __shared__ uint4 s_tile[kFeTile * 2];
  const int f = blockIdx.y;
  const int row = blockIdx.x * kFeQueries + (int)threadIdx.x;
  const FeFrame fr = fe_frame(countsL, countsR, f, capL, capR);
  const bool mine = row >= fr.q0 && row < fr.q1;                      // q1 <= capL
  Top2x32 t2{kNoKey32, kNoKey32};
  const int first = blockIdx.x * kFeQueries;
  if (first < fr.q1 && first + kFeQueries > fr.q0) {                  // block-uniform: some query of this tile is in the range
    D8 q;
    if (mine) q = load_desc(descL + ((size_t)f * capL + row) * 32);
    else {
#pragma unroll
      for (int k = 0; k < 8; k++) q.w[k] = 0;
    }
    const uint4* src = (const uint4*)(descR + (size_t)f * capR * 32);
    for (int tb = fr.t0; tb < fr.t1; tb += tile) {                    // block-uniform, and so are its barriers
      const int n = min(tile, fr.t1 - tb);
      __syncthreads();
      for (int i = threadIdx.x; i < n * 2; i += kFeQueries) s_tile[i] = src[(size_t)tb * 2 + i];
      __syncthreads();
#pragma unroll 4
      for (int c = 0; c < n; c++) {
        const uint4 a = s_tile[2 * c], b = s_tile[2 * c + 1];
        const uint32_t d = __popc(q.w[0] ^ a.x) + __popc(q.w[1] ^ a.y) + __popc(q.w[2] ^ a.z) + __popc(q.w[3] ^ a.w) + __popc(q.w[4] ^ b.x) +
                           __popc(q.w[5] ^ b.y) + __popc(q.w[6] ^ b.z) + __popc(q.w[7] ^ b.w);
        t2 = top2_push(t2, d, (uint32_t)(tb + c));
      }
    }
  }
  if (!mine) t2 = Top2x32{kNoKey32, kNoKey32};
  const int i0 = key_index(t2.k1), i1 = key_index(t2.k2), d0 = key_dist(t2.k1), d1 = key_dist(t2.k2);
  const bool accept = i0 >= 0 && i1 >= 0 && fe_ratio(d0, d1);         // (*it).size() >= 2 && ...
  const unsigned long long word = __ballot(accept);
  const int nwords = (capL + 63) >> 6;
  if ((threadIdx.x & 63) == 0 && (row >> 6) < nwords) words[(size_t)f * nwords + (row >> 6)] = word;
  if (row < capL) {
    const size_t o = ((size_t)f * capL + row) * 2;
    *(int2*)(knn_idx + o) = make_int2(i0, i1);
    *(int2*)(knn_dist + o) = make_int2(d0, d1);
  }
}

__global__ __launch_bounds__(256) void k_fe_compact(const int32_t* __restrict__ countsL, const int32_t* __restrict__ countsR, int capL, int capR,
                                                    const int32_t* __restrict__ knn_idx, const unsigned long long* __restrict__ words,
                                                    orbx_fisheye_pair* __restrict__ pairs, int32_t* __restrict__ npairs) {
  __shared__ int s_wave[4];
  __shared__ int s_base[256];
  __shared__ unsigned long long s_word[256];
  const int f = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const FeFrame fr = fe_frame(countsL, countsR, f, capL, capR);
  const int nwords = (capL + 63) >> 6;
  orbx_fisheye_pair* out = pairs + (size_t)f * capL;
  int carry = 0;
  if (fr.status == 0) {                                               // block-uniform (a frame with a status has no accepted row)
    for (int w0 = 0; w0 < nwords; w0 += 256) {
      const unsigned long long word = w0 + t < nwords ? words[(size_t)f * nwords + w0 + t] : 0ull;
      int total;
      const int base = carry + block_scan<4>(__popcll(word), s_wave, &total);
      s_base[t] = base; s_word[t] = word;
      __syncthreads();
      const int here = min(256, nwords - w0);
      for (int w = wv; w < here; w += 4) {                            // a wave per word: lane b is row (w0 + w) * 64 + b
        const unsigned long long m = s_word[w];
        if ((m >> lane) & 1ull) {
          const int row = (w0 + w) * 64 + lane;
          const int pos = s_base[w] + __popcll(m & ((1ull << lane) - 1ull));
          out[pos] = orbx_fisheye_pair{row, knn_idx[((size_t)f * capL + row) * 2]};
        }
      }
      carry += total;
      __syncthreads();                                                // s_base / s_word are rewritten by the next chunk
    }
  }
  for (int i = carry + t; i < capL; i += 256) out[i] = orbx_fisheye_pair{-1, -1};
  if (t == 0) npairs[f] = fr.status ? fr.status : carry;
}

__global__ __launch_bounds__(256) void k_fe_finish(const orbx_fisheye_pair* __restrict__ pairs, const int32_t* __restrict__ npairs,
                                                   const float* __restrict__ pair_depth, const int32_t* __restrict__ countsL,
                                                   const int32_t* __restrict__ countsR, int capL, int capR, int32_t* __restrict__ l2r,
                                                   int32_t* __restrict__ r2l, float* __restrict__ depth, int32_t* __restrict__ nmatches) {
  __shared__ int s_bad, s_n;
  const int f = blockIdx.x, t = threadIdx.x;
  const FeFrame fr = fe_frame(countsL, countsR, f, capL, capR);
  const int np = npairs[f];
  int status = fr.status;
  if (!status && np < 0) status = np == kFeEmpty ? kFeEmpty : kFeMalformed;
  if (!status && np > capL) status = kFeMalformed;
  const orbx_fisheye_pair* P = pairs + (size_t)f * capL;
  const float* PD = pair_depth + (size_t)f * capL;
  int32_t* L2R = l2r + (size_t)f * capL;
  int32_t* R2L = r2l + (size_t)f * capR;
  float* D = depth + (size_t)f * capL;
  if (t == 0) { s_bad = 0; s_n = 0; }
  for (int i = t; i < capL; i += 256) { L2R[i] = -1; D[i] = -1.0f; }   // :1134, :1136
  for (int i = t; i < capR; i += 256) R2L[i] = -1;                     // :1135
  __syncthreads();                                                     // the -1s are in place before a pair is written over them
  const int nL = fr.q1, nR = fr.t1;                                    // Nleft, Nright
  if (!status) {                                                       // block-uniform
    bool bad = false;
    for (int k = t; k < np; k += 256) {
      const orbx_fisheye_pair p = P[k];
      bad |= p.left < 0 || p.left >= nL || p.right < 0 || p.right >= nR || (k > 0 && P[k - 1].left >= p.left);
    }
    if (bad) s_bad = 1;
    __syncthreads();
    if (s_bad) status = kFeMalformed;
  }
  if (!status) {
    int mine = 0;
    for (int k = t; k < np; k += 256) {
      const orbx_fisheye_pair p = P[k];
      const float d = PD[k];
      if (d > 0.0001f) {                                               // :1157: a NaN fails
        L2R[p.left] = p.right;                                         // the lefts are distinct
        D[p.left] = d;
        atomicMax(&R2L[p.right], p.left);                              // :1159 in pair order: the last = the largest left stays
        mine++;
      }
    }
    if (mine) atomicAdd(&s_n, mine);
    __syncthreads();
  }
  if (t == 0) nmatches[f] = status ? status : s_n;
}

}  // namespace

struct orbx_fisheye : orbx::side::Handle {   // scratch: the ballot words [frames][ceil(capL / 64)]
  orbx_ctx* left = nullptr;
  orbx_ctx* right = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  int tile = kFeTile;                        // ORBX_FISHEYE_TILE at create
};

namespace {

using namespace orbx::side;

int check_batch(orbx_fisheye* h, const std::string& who, int nframes, int capL, int capR) {
  if (nframes < 1) return fail(h, ORBX_E_INVALID, who + "nframes must be at least 1");
  if (capL < 1 || capR < 1 || capL > kFeMaxCap || capR > kFeMaxCap)
    return fail(h, ORBX_E_INVALID, who + "capL and capR must be in 1 .. " + std::to_string(kFeMaxCap));
  if ((long long)nframes * (long long)std::max(capL, capR) > (long long)INT32_MAX / 2)
    return fail(h, ORBX_E_INVALID, who + "nframes * capacity exceeds 2^30");
  return ORBX_OK;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" {

int orbx_fisheye_create(orbx_fisheye** out, orbx_ctx* left, orbx_ctx* right) {
  if (out) *out = nullptr;
  auto bad = [](const char* m, int code = ORBX_E_INVALID) { return create_fail(code, "orbx_fisheye_create", m); };
  if (!out || !left || !right) return bad("null argument");
  if (left == right) return bad("the left and the right side need two contexts");
  if (const char* m = rig_mismatch(left, right)) return bad(m);
  orbx_fisheye* h = new orbx_fisheye();
  h->left = left; h->right = right;
  h->tile = env_int("ORBX_FISHEYE_TILE", 1, kFeTile, kFeTile);
  const char* e = open_handle(h, left->device);
  if (!e && (hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess ||
             hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) != hipSuccess)) {
    (void)hipGetLastError();
    e = "stream / event creation failed";
  }
  if (e) { orbx_fisheye_destroy(h); return bad(e, ORBX_E_DEVICE); }
  *out = h;
  return ORBX_OK;
}

void orbx_fisheye_destroy(orbx_fisheye* h) {
  if (!h) return;
  close_handle(h);
  if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
  if (h->ev_join) (void)hipEventDestroy(h->ev_join);
  delete h;
}

const char* orbx_fisheye_last_error(const orbx_fisheye* h) { return last_error(h); }

int orbx_fisheye_match_batch_device(orbx_fisheye* h, int nframes, int capL, int capR, const uint8_t* d_descL, const int32_t* d_countsL,
                                    const uint8_t* d_descR, const int32_t* d_countsR, int32_t* d_knn_idx, int32_t* d_knn_dist,
                                    orbx_fisheye_pair* d_pairs, int32_t* d_npairs, void* stream) {
  if (!h) return ORBX_E_INVALID;
  const std::string who = "orbx_fisheye_match_batch_device: ";
  int rc = check_batch(h, who, nframes, capL, capR);
  if (rc != ORBX_OK) return rc;
  if (!d_descL || !d_countsL || !d_descR || !d_countsR || !d_knn_idx || !d_knn_dist || !d_pairs || !d_npairs)
    return fail(h, ORBX_E_INVALID, who + "null buffer");
  if (!aligned16(d_descL) || !aligned16(d_descR) || !aligned16(d_knn_idx) || !aligned16(d_knn_dist) || !aligned16(d_pairs))
    return fail(h, ORBX_E_INVALID, who + "the descriptors, the knn tables and the pairs must be 16-byte aligned");
  rc = same_device(h, who.c_str(), {d_descL, d_countsL, d_descR, d_countsR, d_knn_idx, d_knn_dist, d_pairs, d_npairs}, "the rig");
  if (rc != ORBX_OK) return rc;
  ORBX_SIDE_HIP(h, hipSetDevice(h->device));
  const int nwords = (capL + 63) / 64;
  if ((rc = grow(h, &h->scratch, (size_t)nframes * nwords * sizeof(unsigned long long))) != ORBX_OK) return rc;
  unsigned long long* d_words = (unsigned long long*)h->scratch.p;
  hipStream_t st = stream ? (hipStream_t)stream : h->st;
  if ((rc = wait_previous(h, st)) != ORBX_OK) return rc;
  hipLaunchKernelGGL(k_fe_knn, dim3((unsigned)((capL + kFeQueries - 1) / kFeQueries), (unsigned)nframes), dim3(kFeQueries), 0, st, d_descL,
                     d_countsL, d_descR, d_countsR, capL, capR, h->tile, d_knn_idx, d_knn_dist, d_words);
  hipLaunchKernelGGL(k_fe_compact, dim3((unsigned)nframes), dim3(256), 0, st, d_countsL, d_countsR, capL, capR, (const int32_t*)d_knn_idx,
                     (const unsigned long long*)d_words, d_pairs, d_npairs);
  return record_call(h, st);
}

int orbx_fisheye_finish_batch_device(orbx_fisheye* h, int nframes, int capL, int capR, const orbx_fisheye_pair* d_pairs, const int32_t* d_npairs,
                                     const float* d_pair_depth, const int32_t* d_countsL, const int32_t* d_countsR, int32_t* d_l2r,
                                     int32_t* d_r2l, float* d_depth, int32_t* d_nmatches, void* stream) {
  if (!h) return ORBX_E_INVALID;
  const std::string who = "orbx_fisheye_finish_batch_device: ";
  int rc = check_batch(h, who, nframes, capL, capR);
  if (rc != ORBX_OK) return rc;
  if (!d_pairs || !d_npairs || !d_pair_depth || !d_countsL || !d_countsR || !d_l2r || !d_r2l || !d_depth || !d_nmatches)
    return fail(h, ORBX_E_INVALID, who + "null buffer");
  rc = same_device(h, who.c_str(), {d_pairs, d_npairs, d_pair_depth, d_countsL, d_countsR, d_l2r, d_r2l, d_depth, d_nmatches}, "the rig");
  if (rc != ORBX_OK) return rc;
  ORBX_SIDE_HIP(h, hipSetDevice(h->device));
  hipStream_t st = stream ? (hipStream_t)stream : h->st;
  if ((rc = wait_previous(h, st)) != ORBX_OK) return rc;
  hipLaunchKernelGGL(k_fe_finish, dim3((unsigned)nframes), dim3(256), 0, st, d_pairs, d_npairs, d_pair_depth, d_countsL, d_countsR, capL, capR,
                     d_l2r, d_r2l, d_depth, d_nmatches);
  return record_call(h, st);
}

int orbx_fisheye_extract_batch_device(orbx_fisheye* h, const uint8_t* d_imgsL, const uint8_t* d_imgsR, int nframes, int rows, int cols,
                                      size_t row_stride, size_t frame_stride, int lapL0, int lapL1, int lapR0, int lapR1, orbx_keypoint* d_kpsL,
                                      uint8_t* d_descL, int32_t* d_countsL, orbx_keypoint* d_kpsR, uint8_t* d_descR, int32_t* d_countsR,
                                      int32_t* d_knn_idx, int32_t* d_knn_dist, orbx_fisheye_pair* d_pairs, int32_t* d_npairs, void* stream) {
  if (!h) return ORBX_E_INVALID;
  const std::string who = "orbx_fisheye_extract_batch_device: ";
  if (!d_imgsL || !d_imgsR || nframes < 1) return fail(h, ORBX_E_INVALID, who + "no frames");
  if (!d_knn_idx || !d_knn_dist || !d_pairs || !d_npairs) return fail(h, ORBX_E_INVALID, who + "null buffer");
  if (const char* m = rig_mismatch(h->left, h->right)) return fail(h, ORBX_E_INVALID, who + m);
  ORBX_SIDE_HIP(h, hipSetDevice(h->device));
  hipStream_t st = stream ? (hipStream_t)stream : h->left->stream;
  // the right side on the right context's own stream (a NULL stream argument), forked from and joined back into the caller's: the context
  // then remembers no stream of this handle, which may be destroyed before the context
  hipStream_t sr = h->right->stream;
  ORBX_SIDE_HIP(h, hipEventRecord(h->ev_fork, st));
  ORBX_SIDE_HIP(h, hipStreamWaitEvent(sr, h->ev_fork, 0));
  int rc = orbx_extract_batch_device(h->left, d_imgsL, nframes, rows, cols, row_stride, frame_stride, lapL0, lapL1, d_kpsL, d_descL, d_countsL, st);
  if (rc != ORBX_OK) return fail(h, rc, std::string("left extraction: ") + orbx_last_error(h->left));
  rc = orbx_extract_batch_device(h->right, d_imgsR, nframes, rows, cols, row_stride, frame_stride, lapR0, lapR1, d_kpsR, d_descR, d_countsR, nullptr);
  const hipError_t e1 = hipEventRecord(h->ev_join, sr), e2 = hipStreamWaitEvent(st, h->ev_join, 0);   // joined whether or not it succeeded
  if (rc != ORBX_OK) return fail(h, rc, std::string("right extraction: ") + orbx_last_error(h->right));
  ORBX_SIDE_HIP(h, e1);
  ORBX_SIDE_HIP(h, e2);
  const int cap = orbx_keypoint_capacity(h->left);
  return orbx_fisheye_match_batch_device(h, nframes, cap, cap, d_descL, d_countsL, d_descR, d_countsR, d_knn_idx, d_knn_dist, d_pairs, d_npairs, st);
}

int orbx_fisheye_match_batch(orbx_fisheye* h, int nframes, int capL, int capR, const uint8_t* descL, const int32_t* countsL, const uint8_t* descR,
                             const int32_t* countsR, int32_t* knn_idx, int32_t* knn_dist, orbx_fisheye_pair* pairs, int32_t* npairs) {
  if (!h) return ORBX_E_INVALID;
  const std::string who = "orbx_fisheye_match_batch: ";
  int rc = check_batch(h, who, nframes, capL, capR);
  if (rc != ORBX_OK) return rc;
  if (!descL || !countsL || !descR || !countsR || !knn_idx || !knn_dist || !pairs || !npairs) return fail(h, ORBX_E_INVALID, who + "null argument");
  const size_t nl = (size_t)nframes * capL, nr = (size_t)nframes * capR;
  Stager io;
  const size_t o_dL = io.in(descL, nl * 32), o_dR = io.in(descR, nr * 32), o_cL = io.in(countsL, (size_t)nframes * 8),
               o_cR = io.in(countsR, (size_t)nframes * 8);
  const size_t o_i = io.out(knn_idx, nl * 8), o_d = io.out(knn_dist, nl * 8), o_p = io.out(pairs, nl * sizeof(orbx_fisheye_pair)),
               o_n = io.out(npairs, (size_t)nframes * 4);
  if ((rc = upload(h, io)) != ORBX_OK) return rc;
  uint8_t* const d = h->io.p;
  rc = orbx_fisheye_match_batch_device(h, nframes, capL, capR, d + o_dL, (const int32_t*)(d + o_cL), d + o_dR, (const int32_t*)(d + o_cR),
                                       (int32_t*)(d + o_i), (int32_t*)(d + o_d), (orbx_fisheye_pair*)(d + o_p), (int32_t*)(d + o_n), h->st);
  if (rc != ORBX_OK) return rc;
  return download(h, io);
}

int orbx_fisheye_finish_batch(orbx_fisheye* h, int nframes, int capL, int capR, const orbx_fisheye_pair* pairs, const int32_t* npairs,
                              const float* pair_depth, const int32_t* countsL, const int32_t* countsR, int32_t* l2r, int32_t* r2l, float* depth,
                              int32_t* nmatches) {
  if (!h) return ORBX_E_INVALID;
  const std::string who = "orbx_fisheye_finish_batch: ";
  int rc = check_batch(h, who, nframes, capL, capR);
  if (rc != ORBX_OK) return rc;
  if (!pairs || !npairs || !pair_depth || !countsL || !countsR || !l2r || !r2l || !depth || !nmatches)
    return fail(h, ORBX_E_INVALID, who + "null argument");
  const size_t nl = (size_t)nframes * capL, nr = (size_t)nframes * capR;
  Stager io;
  const size_t o_p = io.in(pairs, nl * sizeof(orbx_fisheye_pair)), o_n = io.in(npairs, (size_t)nframes * 4), o_pd = io.in(pair_depth, nl * 4),
               o_cL = io.in(countsL, (size_t)nframes * 8), o_cR = io.in(countsR, (size_t)nframes * 8);
  const size_t o_l = io.out(l2r, nl * 4), o_r = io.out(r2l, nr * 4), o_d = io.out(depth, nl * 4), o_m = io.out(nmatches, (size_t)nframes * 4);
  if ((rc = upload(h, io)) != ORBX_OK) return rc;
  uint8_t* const d = h->io.p;
  rc = orbx_fisheye_finish_batch_device(h, nframes, capL, capR, (const orbx_fisheye_pair*)(d + o_p), (const int32_t*)(d + o_n),
                                        (const float*)(d + o_pd), (const int32_t*)(d + o_cL), (const int32_t*)(d + o_cR), (int32_t*)(d + o_l),
                                        (int32_t*)(d + o_r), (float*)(d + o_d), (int32_t*)(d + o_m), h->st);
  if (rc != ORBX_OK) return rc;
  return download(h, io);
}

}  // extern "C"
