// The batched Fuse search (include/orbx_fuse.h): the window arg-min of ORBmatcher::Fuse (src/ORBmatcher.cc:1148), the Sim3 Fuse (:1340) and
// SearchBySim3 (:1457) for P (query row, keyframe) pairs on the keypoints and descriptors a batch extraction left in HBM.
//
// k_fuse_grid: one workgroup per keyframe.  Cell of every keypoint (Frame::PosInGrid), a count per cell in LDS, a scan of the 3072 cells,
//   an unordered fill of each cell's segment and then, a thread per entry, the entry's rank inside its segment (how many of the segment's
//   indices are smaller): the list sorted by (cell, index).  It is kept as 16-byte records {x, y, octave, uright} with the features' indices
//   beside them: a candidate's position in the list is its place in GetFeaturesInArea's walk (ix major, iy minor, insertion order), and the
//   cells of one ix column are one contiguous segment.
// k_fuse_check: one workgroup per pair.  The pair's keyframe, its grid, nquery and every query's `point` are checked before any of them
//   addresses memory; the verdict {keyframe or -1, nquery} goes to the handle's memory and d_nfound[p] becomes 0 or -1.
// k_fuse_search<LDS>: one workgroup per chunk of kQ queries of one pair, A LANE PER QUERY: a window holds 3 - 10 candidates, which leaves a
//   wave per query idle, and with a lane per query neither the running best nor the walk-order tie rule crosses
//   lanes.  The query's descriptor stays in 8 registers.  LDS path: the keyframe's cell starts, records, indices and descriptors are staged
//   by 16-byte LDS-DMA loads (12 304 + 52 capacity bytes); global path (keyframes that need more than the handle's limit): the same arrays
//   where they lie.  The large pair (every neighbour's points against the new keyframe) is many chunks, hence many workgroups.  The hits are
//   counted by ballot, one LDS add per wave and one global add per workgroup on d_nfound[p]; integer adds, so the order does not matter.
// The float expressions are compiled with -ffp-contract=off: every operation is rounded by itself, as the specification states them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <string>

#include "../side/orbx_handle.h"
#include "../side/orbx_pair_device.h"
#include "../../../include/orbx_fuse.h"

namespace {

using namespace orbx::side::dev;

constexpr int kCols = 64, kRows = 48, kCells = kCols * kRows;
constexpr int kCsStride = kCells + 4;     // cell starts of one keyframe: 3073 entries, padded to a multiple of 16 bytes
constexpr int kGridThreads = 1024;        // 3 cells a thread in the scan
constexpr int kCheckThreads = 256;
constexpr int kQ = 512;                   // queries (lanes) of one workgroup of k_fuse_search
constexpr int kLdsMax = 152 * 1024;       // dynamic LDS of one workgroup (160 KiB per CU, the static part is below 1 KiB)
static_assert(kCells == 3 * kGridThreads && (kCsStride * 4) % 16 == 0, "the scan's and the staging's shapes");

constexpr size_t kX = offsetof(orbx_keypoint, x), kY = offsetof(orbx_keypoint, y), kOctave = offsetof(orbx_keypoint, octave);

struct __align__(16) Hdr {               // a keyframe's grid
  int32_t n, nin, omin, omax;            // count (-1: no grid), features in cells, their octaves' range
  float min_x, min_y, inv_w, inv_h;
};

struct GridArgs {
  const uint8_t* kps; const int32_t* counts; const float* uright; const float* parm;
  Hdr* hdr; int32_t* cs; Rec* recs; int32_t* idx; int32_t* tmp;
  int cap, cap4;
};

// Frame::PosInGrid (src/Frame.cc:725-735): the cell id ix * 48 + iy, -1 for a feature in no cell
__device__ __forceinline__ int cell_of(const uint8_t* kp, int i, float min_x, float min_y, float inv_w, float inv_h) {
  const float px = (kp_field<float>(kp, i, kX) - min_x) * inv_w;
  const float py = (kp_field<float>(kp, i, kY) - min_y) * inv_h;
  if (!(fabsf(px) < 1e9f) || !(fabsf(py) < 1e9f)) return -1;   // NaN, infinite or far outside: not converted
  const int posX = (int)roundf(px), posY = (int)roundf(py);
  return (posX < 0 || posX >= kCols || posY < 0 || posY >= kRows) ? -1 : posX * kRows + posY;
}

__global__ __launch_bounds__(kGridThreads) void k_fuse_grid(GridArgs g) {
  __shared__ int s_start[kCells + 1], s_fill[kCells], s_wsum[kGridThreads / 64], s_omin, s_omax;
  const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = g.counts[2 * k];
  if (n < 0 || n > g.cap) {                // uniform over the workgroup
    if (tid == 0) g.hdr[k] = Hdr{-1, 0, 0, 0, 0.0f, 0.0f, 0.0f, 0.0f};
    return;
  }
  const uint8_t* const kp = g.kps + (size_t)k * g.cap * sizeof(orbx_keypoint);
  const float min_x = g.parm[4 * k], min_y = g.parm[4 * k + 1], inv_w = g.parm[4 * k + 2], inv_h = g.parm[4 * k + 3];
  int32_t* const cs = g.cs + (size_t)k * kCsStride;
  int32_t* const tmp = g.tmp + (size_t)k * g.cap4;
  for (int c = tid; c < kCells; c += kGridThreads) s_fill[c] = 0;
  if (tid == 0) { s_omin = INT_MAX; s_omax = INT_MIN; }
  __syncthreads();
  // ---- a count per cell
  for (int i = tid; i < n; i += kGridThreads) {
    const int c = cell_of(kp, i, min_x, min_y, inv_w, inv_h);
    if (c >= 0) {
      atomicAdd(&s_fill[c], 1);
      const int o = kp_field<int32_t>(kp, i, kOctave);
      atomicMin(&s_omin, o); atomicMax(&s_omax, o);
    }
  }
  __syncthreads();
  // ---- the scan: 3 cells a thread, a shuffle scan inside the wave, the 16 wave sums through LDS
  const int a0 = s_fill[3 * tid], a1 = s_fill[3 * tid + 1], a2 = s_fill[3 * tid + 2];
  const int mine = a0 + a1 + a2;
  int inc = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(inc, o); if (lane >= o) inc += u; }
  if (lane == 63) s_wsum[wave] = inc;
  __syncthreads();
  int off = 0, total = 0;
#pragma unroll
  for (int w = 0; w < kGridThreads / 64; w++) { const int s = s_wsum[w]; if (w < wave) off += s; total += s; }
  const int excl = off + inc - mine;
  s_start[3 * tid] = excl; s_start[3 * tid + 1] = excl + a0; s_start[3 * tid + 2] = excl + a0 + a1;
  if (tid == 0) s_start[kCells] = total;
  s_fill[3 * tid] = 0; s_fill[3 * tid + 1] = 0; s_fill[3 * tid + 2] = 0;
  __syncthreads();
  for (int c = tid; c < kCsStride; c += kGridThreads) cs[c] = s_start[min(c, kCells)];
  // ---- each cell's segment, in whatever order the atomics give
  for (int i = tid; i < n; i += kGridThreads) {
    const int c = cell_of(kp, i, min_x, min_y, inv_w, inv_h);
    if (c >= 0) tmp[s_start[c] + atomicAdd(&s_fill[c], 1)] = i;
  }
  __syncthreads();                         // tmp is read by other threads of this workgroup
  // ---- the stable order: an entry's place in its segment is the number of smaller indices there
  const float* const ur = g.uright ? g.uright + (size_t)k * g.cap : nullptr;
  Rec* const recs = g.recs + (size_t)k * g.cap;
  int32_t* const idx = g.idx + (size_t)k * g.cap4;
  for (int pos = tid; pos < total; pos += kGridThreads) {
    const int i = tmp[pos];
    const int c = cell_of(kp, i, min_x, min_y, inv_w, inv_h);
    const int b = s_start[c], e = s_start[c + 1];
    int rank = 0;
    for (int j = b; j < e; j++) rank += tmp[j] < i;
    recs[b + rank] = Rec{kp_field<float>(kp, i, kX), kp_field<float>(kp, i, kY), kp_field<int32_t>(kp, i, kOctave), ur ? ur[i] : -1.0f};
    idx[b + rank] = i;
  }
  if (tid == 0) g.hdr[k] = Hdr{n, total, s_omin, s_omax, min_x, min_y, inv_w, inv_h};
}

struct CheckArgs {
  const Hdr* hdr; const orbx_fuse_query* query; const int32_t* nquery; const int32_t* pairs;
  int2* pst; int32_t* nfound;
  int nframes, qcap, npoints, gate, nlevels;
};

__global__ __launch_bounds__(kCheckThreads) void k_fuse_check(CheckArgs g) {
  __shared__ int s_bad;
  const int p = blockIdx.x, tid = threadIdx.x;
  const int k = g.pairs[p], nq = g.nquery[p];
  bool ok = k >= 0 && k < g.nframes && nq >= 0 && nq <= g.qcap;
  if (ok) {
    const Hdr h = g.hdr[k];
    ok = h.n >= 0 && !(g.gate && h.nin > 0 && (h.omin < 0 || h.omax >= g.nlevels));
  }
  if (tid == 0) s_bad = 0;
  __syncthreads();
  if (ok) {                                // uniform over the workgroup
    const orbx_fuse_query* const row = g.query + (size_t)p * g.qcap;
    bool bad = false;
    for (int q = tid; q < nq; q += kCheckThreads) bad |= row[q].point >= g.npoints;
    if (bad) s_bad = 1;
  }
  __syncthreads();
  if (tid == 0) {
    ok = ok && !s_bad;
    g.pst[p] = ok ? make_int2(k, nq) : make_int2(-1, 0);
    g.nfound[p] = ok ? 0 : -1;
  }
}

struct SearchArgs {
  const uint8_t* desc; const Hdr* hdr; const int32_t* cs; const Rec* recs; const int32_t* idx;
  const orbx_fuse_query* query; const int2* pst; const uint8_t* pdesc;
  int32_t* bidx; int32_t* bdist; int32_t* nfound;
  int cap, cap4, qcap, nchunks, gate, th_low;
  float inv[ORBX_FUSE_MAX_LEVELS];
};

__host__ __device__ inline size_t lds_bytes(int cap) { return (size_t)kCsStride * 4 + (size_t)cap * 48 + (size_t)((cap + 3) & ~3) * 4; }

template <bool LDS>
__global__ __launch_bounds__(kQ) void k_fuse_search(SearchArgs g) {
  extern __shared__ __align__(16) uint8_t smem[];
  __shared__ int s_cnt;
  __shared__ float s_inv[ORBX_FUSE_MAX_LEVELS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int p = blockIdx.x / g.nchunks, chunk = blockIdx.x - p * g.nchunks;
  const int q = chunk * kQ + tid;
  const size_t row = (size_t)p * g.qcap;
  const int2 st = g.pst[p];                // the verdict of k_fuse_check: both values are in range
  const int k = st.x, nq = st.y;
  if (k < 0 || chunk * kQ >= nq) {         // uniform over the workgroup: a malformed pair, or a chunk past the row's queries
    if (q < g.qcap) { g.bidx[row + q] = -1; g.bdist[row + q] = 256; }
    return;
  }
  if (tid < ORBX_FUSE_MAX_LEVELS) {        // the level table: constant indices into the kernel's arguments
    float v = 0.0f;
#pragma unroll
    for (int l = 0; l < ORBX_FUSE_MAX_LEVELS; l++)
      if (tid == l) v = g.inv[l];
    s_inv[tid] = v;
  }
  if (tid == 0) s_cnt = 0;
  const Hdr h = g.hdr[k];
  // LDS: cell starts | records | indices | descriptors
  int32_t* const l_cs = (int32_t*)smem;
  Rec* const l_recs = (Rec*)(smem + (size_t)kCsStride * 4);
  int32_t* const l_idx = (int32_t*)((uint8_t*)l_recs + (size_t)g.cap * 16);
  uint8_t* const l_desc = (uint8_t*)l_idx + (size_t)g.cap4 * 4;
  const int32_t* const gcs = g.cs + (size_t)k * kCsStride;
  const Rec* const grecs = g.recs + (size_t)k * g.cap;
  const int32_t* const gidx = g.idx + (size_t)k * g.cap4;
  const uint8_t* const gdesc = g.desc + (size_t)k * g.cap * 32;
  if (LDS) {
    stage_dma<kQ>((uint8_t*)l_cs, (const uint8_t*)gcs, kCsStride / 4);
    stage_dma<kQ>((uint8_t*)l_recs, (const uint8_t*)grecs, h.nin);
    stage_dma<kQ>((uint8_t*)l_idx, (const uint8_t*)gidx, (h.nin + 3) >> 2);
    stage_dma<kQ>(l_desc, gdesc, h.n * 2);
  }
  // this instantiation's arrays: LDS or global, decided at compile time
  const int32_t* const cs = LDS ? l_cs : gcs;
  const Rec* const recs = LDS ? l_recs : grecs;
  const int32_t* const idx = LDS ? l_idx : gidx;
  const uint8_t* const desc = LDS ? l_desc : gdesc;

  // ---- the lane's query
  float x = 0.0f, y = 0.0f, r = 0.0f, qur = 0.0f;
  int min_level = 0, max_level = -1;
  bool valid = false;
  D8 qd;
#pragma unroll
  for (int w = 0; w < 8; w++) qd.w[w] = 0;
  if (q < nq) {
    const uint4* const rq = (const uint4*)(g.query + row + q);
    const uint4 lo = rq[0], hi = rq[1];
    x = __uint_as_float(lo.x); y = __uint_as_float(lo.y); r = __uint_as_float(lo.z); qur = __uint_as_float(lo.w);
    min_level = (int)hi.x; max_level = (int)hi.y;
    const int point = (int)hi.z;           // below npoints: k_fuse_check
    valid = point >= 0 && fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(r) < INFINITY;   // a NaN fails every comparison
    if (valid) qd = load_desc(g.pdesc + (size_t)point * 32);
  }
  if (LDS) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the LDS-DMA loads have landed
  __syncthreads();

  int best = 256, bi = -1;
  if (valid) {
    // KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:704-748) with its four early returns
    const int nMinCellX = max(0, (int)floorf((x - h.min_x - r) * h.inv_w));
    const int nMaxCellX = min(kCols - 1, (int)ceilf((x - h.min_x + r) * h.inv_w));
    const int nMinCellY = max(0, (int)floorf((y - h.min_y - r) * h.inv_h));
    const int nMaxCellY = min(kRows - 1, (int)ceilf((y - h.min_y + r) * h.inv_h));
    if (nMinCellX < kCols && nMaxCellX >= 0 && nMinCellY < kRows && nMaxCellY >= 0 && nMinCellY <= nMaxCellY) {
      for (int ix = nMinCellX; ix <= nMaxCellX; ix++) {
        // the cells iy = nMinCellY .. nMaxCellY of column ix are one segment of the list
        const int j1 = cs[ix * kRows + nMaxCellY + 1];
        for (int j = cs[ix * kRows + nMinCellY]; j < j1; j++) {
          const Rec c = recs[j];
          if (c.octave < min_level || c.octave > max_level) continue;
          const float distx = c.x - x, disty = c.y - y;
          if (!(fabsf(distx) < r && fabsf(disty) < r)) continue;
          if (g.gate) {                    // src/ORBmatcher.cc:1272-1296; the octave is a level: k_fuse_check
            const float ex = x - c.x, ey = y - c.y;
            if (c.ur >= 0.0f) {
              const float er = qur - c.ur;
              const float e2 = ex * ex + ey * ey + er * er;
              if ((double)(e2 * s_inv[c.octave]) > 7.8) continue;
            } else {
              const float e2 = ex * ex + ey * ey;
              if ((double)(e2 * s_inv[c.octave]) > 5.99) continue;
            }
          }
          const int i = idx[j];
          const int d = hamming(qd, load_desc(desc + (size_t)i * 32));
          if (d < best) { best = d; bi = i; }
        }
      }
    }
  }
  if (q < g.qcap) { g.bidx[row + q] = bi; g.bdist[row + q] = best; }
  const int hits = __popcll(__ballot(bi >= 0 && best <= g.th_low));
  if (lane == 0 && hits) atomicAdd(&s_cnt, hits);
  __syncthreads();
  if (tid == 0 && s_cnt) atomicAdd(g.nfound + p, s_cnt);
}

}  // namespace

struct orbx_fuse : orbx::side::Handle {       // scratch: the grids of `built`
  int lds_limit = kLdsMax;                    // ORBX_FUSE_LDS at create
  orbx::side::Block pst;                      // the pairs' verdicts of the call in flight
  bool have_grids = false;
  orbx_fuse_side built = {};                  // the side the grids were built from
  size_t o_hdr = 0, o_cs = 0, o_recs = 0, o_idx = 0;
};

namespace {

using namespace orbx::side;

const char* side_problem(const orbx_fuse_side* s) {
  if (!s) return "null side";
  if (s->nframes < 1 || s->capacity < 1) return "nframes and capacity must be at least 1";
  if (s->capacity > ORBX_FUSE_MAX_CAPACITY) return "capacity above 32768";
  if (!s->d_kps || !s->d_desc || !s->d_counts || !s->d_gridparm) return "null buffer in the side";
  if ((long long)s->nframes * ((long long)s->capacity + 4) > (long long)INT_MAX) return "nframes * capacity exceeds INT_MAX";
  return nullptr;
}

bool same_side(const orbx_fuse_side& a, const orbx_fuse_side& b) {
  return a.d_kps == b.d_kps && a.d_desc == b.d_desc && a.d_counts == b.d_counts && a.d_uright == b.d_uright && a.d_gridparm == b.d_gridparm &&
         a.nframes == b.nframes && a.capacity == b.capacity;
}

// what both forms of the search check before anything is copied or launched
int check_search(orbx_fuse* m, const char* who, const orbx_fuse_side* side, const void* query, const void* nquery, int qcap, const void* pairs,
                 int npairs, const void* pdesc, int npoints, const float* inv, int nlevels, int gate, const void* bidx, const void* bdist,
                 const void* nfound) {
  if (const char* e = side_problem(side)) return fail(m, ORBX_E_INVALID, std::string(who) + e);
  if (!query || !nquery || !pairs || !pdesc) return fail(m, ORBX_E_INVALID, std::string(who) + "null query, nquery, pairs or pdesc");
  if (!bidx || !bdist || !nfound) return fail(m, ORBX_E_INVALID, std::string(who) + "null best_idx, best_dist or nfound");
  if (qcap < 1 || npairs < 1 || npoints < 1)
    return fail(m, ORBX_E_INVALID, std::string(who) + "qcap, npairs and npoints must be at least 1");
  if (gate && (!inv || nlevels < 1 || nlevels > ORBX_FUSE_MAX_LEVELS))
    return fail(m, ORBX_E_INVALID, std::string(who) + "the gate needs inv_level_sigma2 and nlevels in 1 .. 16 (nlevels = " + std::to_string(nlevels) + ")");
  if ((long long)npairs * ((long long)qcap + kQ) > (long long)INT_MAX)
    return fail(m, ORBX_E_INVALID, std::string(who) + "npairs * qcap exceeds INT_MAX");
  return ORBX_OK;
}

}  // namespace

extern "C" {

int orbx_fuse_create(orbx_fuse** out, int device) {
  return create_handle(out, device, "orbx_fuse_create", orbx_fuse_destroy, [](orbx_fuse* m) {
    m->lds_limit = env_int("ORBX_FUSE_LDS", 0, kLdsMax, kLdsMax);
    return allow_lds((const void*)k_fuse_search<true>, kLdsMax);
  });
}

void orbx_fuse_destroy(orbx_fuse* m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  if (m->pending && m->ev_done) (void)hipEventSynchronize(m->ev_done);
  if (m->pst.p) (void)hipFree(m->pst.p);
  close_handle(m);
  delete m;
}

const char* orbx_fuse_last_error(const orbx_fuse* m) { return last_error(m); }

int orbx_fuse_grids_device(orbx_fuse* m, const orbx_fuse_side* side, void* stream) {
  if (!m) return ORBX_E_INVALID;
  const char* who = "orbx_fuse_grids_device: ";
  if (const char* e = side_problem(side)) return fail(m, ORBX_E_INVALID, std::string(who) + e);
  int rc = same_device(m, who, {side->d_kps, side->d_desc, side->d_counts, side->d_uright, side->d_gridparm}, "the handle");
  if (rc != ORBX_OK) return rc;
  ORBX_SIDE_HIP(m, hipSetDevice(m->device));
  m->have_grids = false;
  const size_t K = (size_t)side->nframes, cap = (size_t)side->capacity, cap4 = (cap + 3) & ~(size_t)3;
  Layout lay;
  m->o_hdr = lay.add(K * sizeof(Hdr));
  m->o_cs = lay.add(K * kCsStride * 4);
  m->o_recs = lay.add(K * cap * sizeof(Rec));
  m->o_idx = lay.add(K * cap4 * 4);
  const size_t o_tmp = lay.add(K * cap4 * 4);
  if ((rc = grow(m, &m->scratch, lay.size)) != ORBX_OK) return rc;
  uint8_t* const d = m->scratch.p;
  GridArgs g;
  g.kps = (const uint8_t*)side->d_kps; g.counts = side->d_counts; g.uright = side->d_uright; g.parm = side->d_gridparm;
  g.hdr = (Hdr*)(d + m->o_hdr); g.cs = (int32_t*)(d + m->o_cs); g.recs = (Rec*)(d + m->o_recs); g.idx = (int32_t*)(d + m->o_idx);
  g.tmp = (int32_t*)(d + o_tmp);
  g.cap = (int)cap; g.cap4 = (int)cap4;
  hipStream_t st = stream ? (hipStream_t)stream : m->st;
  if ((rc = wait_previous(m, st)) != ORBX_OK) return rc;
  hipLaunchKernelGGL(k_fuse_grid, dim3((unsigned)K), dim3(kGridThreads), 0, st, g);
  if ((rc = record_call(m, st)) != ORBX_OK) return rc;
  m->built = *side;
  m->have_grids = true;
  return ORBX_OK;
}

int orbx_fuse_search_device(orbx_fuse* m, const orbx_fuse_side* side, const orbx_fuse_query* d_query, const int32_t* d_nquery, int qcap,
                            const int32_t* d_pairs, int npairs, const uint8_t* d_pdesc, int npoints, const float* inv_level_sigma2, int nlevels,
                            int reprojection_gate, int th_low, int32_t* d_best_idx, int32_t* d_best_dist, int32_t* d_nfound, void* stream) {
  if (!m) return ORBX_E_INVALID;
  const char* who = "orbx_fuse_search_device: ";
  int rc = check_search(m, who, side, d_query, d_nquery, qcap, d_pairs, npairs, d_pdesc, npoints, inv_level_sigma2, nlevels, reprojection_gate,
                        d_best_idx, d_best_dist, d_nfound);
  if (rc != ORBX_OK) return rc;
  if (!m->have_grids || !same_side(m->built, *side))
    return fail(m, ORBX_E_INVALID, std::string(who) + "no grids of this side on the handle: call orbx_fuse_grids_device first");
  rc = same_device(m, who, {side->d_desc, d_query, d_nquery, d_pairs, d_pdesc, d_best_idx, d_best_dist, d_nfound}, "the handle");
  if (rc != ORBX_OK) return rc;
  ORBX_SIDE_HIP(m, hipSetDevice(m->device));
  if ((rc = grow(m, &m->pst, (size_t)npairs * sizeof(int2))) != ORBX_OK) return rc;
  const uint8_t* const d = m->scratch.p;
  const int cap = side->capacity;
  CheckArgs c;
  c.hdr = (const Hdr*)(d + m->o_hdr); c.query = d_query; c.nquery = d_nquery; c.pairs = d_pairs;
  c.pst = (int2*)m->pst.p; c.nfound = d_nfound;
  c.nframes = side->nframes; c.qcap = qcap; c.npoints = npoints; c.gate = reprojection_gate != 0; c.nlevels = nlevels;
  SearchArgs g;
  g.desc = side->d_desc; g.hdr = c.hdr; g.cs = (const int32_t*)(d + m->o_cs); g.recs = (const Rec*)(d + m->o_recs);
  g.idx = (const int32_t*)(d + m->o_idx);
  g.query = d_query; g.pst = c.pst; g.pdesc = d_pdesc;
  g.bidx = d_best_idx; g.bdist = d_best_dist; g.nfound = d_nfound;
  g.cap = cap; g.cap4 = (cap + 3) & ~3; g.qcap = qcap; g.nchunks = (qcap + kQ - 1) / kQ; g.gate = c.gate; g.th_low = th_low;
  for (int l = 0; l < ORBX_FUSE_MAX_LEVELS; l++) g.inv[l] = (c.gate && l < nlevels) ? inv_level_sigma2[l] : 0.0f;
  const size_t lds = lds_bytes(cap);
  const unsigned blocks = (unsigned)npairs * (unsigned)g.nchunks;
  hipStream_t st = stream ? (hipStream_t)stream : m->st;
  if ((rc = wait_previous(m, st)) != ORBX_OK) return rc;
  hipLaunchKernelGGL(k_fuse_check, dim3((unsigned)npairs), dim3(kCheckThreads), 0, st, c);
  if (lds <= (size_t)m->lds_limit) hipLaunchKernelGGL(k_fuse_search<true>, dim3(blocks), dim3(kQ), lds, st, g);
  else hipLaunchKernelGGL(k_fuse_search<false>, dim3(blocks), dim3(kQ), 0, st, g);
  return record_call(m, st);
}

int orbx_fuse_search(orbx_fuse* m, const orbx_fuse_side* side, const orbx_fuse_query* query, const int32_t* nquery, int qcap,
                     const int32_t* pairs, int npairs, const uint8_t* pdesc, int npoints, const float* inv_level_sigma2, int nlevels,
                     int reprojection_gate, int th_low, int32_t* best_idx, int32_t* best_dist, int32_t* nfound) {
  if (!m) return ORBX_E_INVALID;
  const char* who = "orbx_fuse_search: ";
  int rc = check_search(m, who, side, query, nquery, qcap, pairs, npairs, pdesc, npoints, inv_level_sigma2, nlevels, reprojection_gate, best_idx,
                        best_dist, nfound);
  if (rc != ORBX_OK) return rc;
  Stager io;
  const size_t nf = (size_t)side->nframes, nk = nf * side->capacity, rows = (size_t)npairs * qcap;
  const size_t o_kps = io.in(side->d_kps, nk * sizeof(orbx_keypoint)), o_desc = io.in(side->d_desc, nk * 32), o_counts = io.in(side->d_counts, nf * 8);
  const size_t o_ur = side->d_uright ? io.in(side->d_uright, nk * 4) : 0, o_parm = io.in(side->d_gridparm, nf * 16);
  const size_t o_query = io.in(query, rows * sizeof(orbx_fuse_query)), o_nq = io.in(nquery, (size_t)npairs * 4);
  const size_t o_pairs = io.in(pairs, (size_t)npairs * 4), o_pdesc = io.in(pdesc, (size_t)npoints * 32);
  const size_t o_bi = io.out(best_idx, rows * 4), o_bd = io.out(best_dist, rows * 4), o_nf = io.out(nfound, (size_t)npairs * 4);
  if ((rc = upload(m, io)) != ORBX_OK) return rc;
  uint8_t* const d = m->io.p;
  const orbx_fuse_side ds = {(const orbx_keypoint*)(d + o_kps), d + o_desc, (const int32_t*)(d + o_counts),
                             side->d_uright ? (const float*)(d + o_ur) : nullptr, (const float*)(d + o_parm), side->nframes, side->capacity};
  if ((rc = orbx_fuse_grids_device(m, &ds, m->st)) != ORBX_OK) return rc;
  rc = orbx_fuse_search_device(m, &ds, (const orbx_fuse_query*)(d + o_query), (const int32_t*)(d + o_nq), qcap, (const int32_t*)(d + o_pairs), npairs,
                               d + o_pdesc, npoints, inv_level_sigma2, nlevels, reprojection_gate, th_low, (int32_t*)(d + o_bi), (int32_t*)(d + o_bd),
                               (int32_t*)(d + o_nf), m->st);
  if (rc != ORBX_OK) return rc;
  return download(m, io);
}

}  // extern "C"
