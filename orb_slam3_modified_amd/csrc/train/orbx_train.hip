// Vocabulary training (include/orbx_train.h): DBoW2's TemplatedVocabulary::create (TemplatedVocabulary.h:558-616) — hierarchical k-means++
// over binary descriptors, createWords, setNodeWeights — bit-exact, with the k-means of the large nodes on the GPU.
//
// The draw order forces the reference's depth-first walk: a node's k-means++ seeding draws from the one glibc rand() stream, and how many
// draws a subtree takes depends on its data, so nodes are processed one at a time in HKmeansStep's order (:642-822).  The parallelism is inside
// a node: its n descriptors against <= 20 centres, the bit counts of the means, the prefix scans and the stable partition.  A node's
// descriptors are a contiguous range; its children's ranges are the stable partition of it by final cluster, so every child keeps the
// reference's per-node order (`groups[i]` lists indices ascending).  Two buffers alternate by level: a node at level l reads buffer (l-1)&1 and
// writes its children's ranges, at the same offsets, into buffer l&1.  Nodes with at least device_min_node descriptors run here on the GPU,
// the others (the bottom levels: ~10^5 nodes of 10-100 descriptors) in a tight host loop; no launch pays for those.
//
// Exactness: distances are integers 0..256; every double running sum of the seeding is an integer below 2^53, so an int64 prefix compared
// with ceil(cut) picks the reference's index; bit counts are integers.  No reduction order can change a result.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/orbx_train.h"

namespace {

thread_local std::string g_err;

// ---- glibc rand() (TYPE_3: the additive feedback generator of random_r.c, x[i] = x[i-3] + x[i-31]) --------------------------------------
struct GlibcRand {
  int32_t r[31];
  int f = 3, b = 0;
  explicit GlibcRand(uint32_t seed) {
    int32_t word = seed == 0 ? 1 : (int32_t)seed;   // srandom_r: seed 0 -> 1, the state words are int32_t
    r[0] = word;
    for (int i = 1; i < 31; i++) {   // word = 16807 * word % 2147483647 by Schrage's method, as random_r.c computes it
      const int64_t hi = word / 127773, lo = word % 127773;
      int64_t w = 16807 * lo - 2836 * hi;
      if (w < 0) w += 2147483647;
      word = (int32_t)w;
      r[i] = word;
    }
    for (int i = 0; i < 310; i++) next();
  }
  int32_t next() {
    const uint32_t v = (uint32_t)r[f] + (uint32_t)r[b];
    r[f] = (int32_t)v;
    const int32_t out = (int32_t)(v >> 1);
    if (++f >= 31) f = 0;
    if (++b >= 31) b = 0;
    return out;
  }
  // DUtils::Random::RandomInt (Random.cpp:47-50)
  int random_int(int mn, int mx) {
    const int d = mx - mn + 1;
    return int(((double)next() / ((double)RAND_MAX + 1.0)) * d) + mn;
  }
  // DUtils::Random::RandomValue<double>(min, max) (Random.h:56-69)
  double random_value(double mn, double mx) { return (double)next() / (double)RAND_MAX * (mx - mn) + mn; }
};

inline int hamming4(const uint64_t* a, const uint64_t* b) {
  return __builtin_popcountll(a[0] ^ b[0]) + __builtin_popcountll(a[1] ^ b[1]) + __builtin_popcountll(a[2] ^ b[2]) +
         __builtin_popcountll(a[3] ^ b[3]);
}

// byte p of kSpread[v] = bit p of v: 32 byte-lane additions per descriptor count all 256 bits (flushed before a lane can reach 256)
struct Spread {
  uint64_t t[256];
  Spread() {
    for (int v = 0; v < 256; v++) {
      uint64_t x = 0;
      for (int p = 0; p < 8; p++) x |= (uint64_t)((v >> p) & 1) << (8 * p);
      t[v] = x;
    }
  }
};
const Spread kSpread;

// ---- device kernels: one node's range, 256 descriptors per block ------------------------------------------------------------------------
constexpr int kMaxK = 20;
constexpr int kBlock = 256;

__device__ inline int dev_hamming(const ulonglong4& x, const uint64_t* c) {
  return __popcll(x.x ^ c[0]) + __popcll(x.y ^ c[1]) + __popcll(x.z ^ c[2]) + __popcll(x.w ^ c[3]);
}

// seeding step 2: md[i] = min(md[i], H(x_i, c)) (first: = H), the block's int64 sum, and the total (atomic: integers, any order)
__global__ __launch_bounds__(kBlock) void k_seed_dist(const ulonglong4* __restrict__ x, int n, const uint64_t* __restrict__ centre, int first,
                                                        int* __restrict__ md, long long* __restrict__ bsum, unsigned long long* __restrict__ total) {
  __shared__ long long part[kBlock / 64];
  const int i = blockIdx.x * kBlock + threadIdx.x;
  long long v = 0;
  if (i < n) {
    const int d = dev_hamming(x[i], centre);
    const int m = first ? d : min(md[i], d);
    md[i] = m;
    v = m;
  }
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    const long long s = part[0] + part[1] + part[2] + part[3];
    bsum[blockIdx.x] = s;
    atomicAdd(total, (unsigned long long)s);
  }
}

// block-wide inclusive scan of one int64 per thread (256 threads)
__device__ inline long long block_scan_incl(long long v, long long* lds /* [kBlock/64] */) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int o = 1; o < 64; o <<= 1) {
    const long long t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  if (lane == 63) lds[w] = v;
  __syncthreads();
  long long base = 0;
  for (int j = 0; j < w; j++) base += lds[j];
  __syncthreads();
  return v + base;
}

// seeding step 3: the first index whose running sum reaches `cut` (= ceil of the reference's double cut: the sums are exact integers);
// one workgroup: the block sums locate the block, then the block's own entries.  Writes the chosen descriptor as centre `slot`.
__global__ __launch_bounds__(kBlock) void k_seed_select(const ulonglong4* __restrict__ x, int n, const int* __restrict__ md,
                                                          const long long* __restrict__ bsum, int nb, long long cut, ulonglong4* __restrict__ cent,
                                                          int slot) {
  __shared__ long long lds[kBlock / 64];
  __shared__ int found;
  __shared__ long long base_s, chunk_end;
  const int t = threadIdx.x;
  if (t == 0) found = INT_MAX;
  __syncthreads();
  long long base = 0;
  int blk = -1;
  for (int c0 = 0; c0 < nb; c0 += kBlock) {   // every branch below is workgroup-uniform (`found` is read after a barrier)
    const int j = c0 + t;
    const long long v = j < nb ? bsum[j] : 0;
    const long long incl = block_scan_incl(v, lds) + base;
    if (j < nb && incl >= cut) atomicMin(&found, j);
    if (t == kBlock - 1) chunk_end = incl;
    __syncthreads();
    if (found != INT_MAX) {
      if (j == found) base_s = incl - v;
      __syncthreads();
      blk = found;
      base = base_s;
      break;
    }
    base = chunk_end;
    __syncthreads();
  }
  if (blk < 0) {   // cannot happen (cut <= sum); the reference's fallback, :899-900
    if (t == 0) cent[slot] = x[n - 1];
    return;
  }
  __syncthreads();
  if (t == 0) found = INT_MAX;
  __syncthreads();
  const int i = blk * kBlock + t;
  const long long incl = block_scan_incl(i < n ? md[i] : 0, lds) + base;
  if (i < n && incl >= cut) atomicMin(&found, i);
  __syncthreads();
  if (t == 0) cent[slot] = x[found < n ? found : n - 1];
}

// assignment: argmin over the centres in index order with a strict < (the lowest index wins a tie), the "changed" flag against the
// previous association and the cluster sizes
__global__ __launch_bounds__(kBlock) void k_assign(const ulonglong4* __restrict__ x, int n, const ulonglong4* __restrict__ cent, int kc,
                                                     int first, int* __restrict__ assoc, int* __restrict__ changed, int* __restrict__ sizes) {
  __shared__ uint64_t c[kMaxK * 4];
  __shared__ int hist[kMaxK];
  if (threadIdx.x < kc * 4) c[threadIdx.x] = ((const uint64_t*)cent)[threadIdx.x];
  if (threadIdx.x < kMaxK) hist[threadIdx.x] = 0;
  __syncthreads();
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) {
    const ulonglong4 v = x[i];
    int best = dev_hamming(v, c), bi = 0;
    for (int j = 1; j < kc; j++) {
      const int d = dev_hamming(v, c + 4 * j);
      if (d < best) { best = d; bi = j; }
    }
    if (!first && assoc[i] != bi) *changed = 1;
    assoc[i] = bi;
    atomicAdd(&hist[bi], 1);
  }
  __syncthreads();
  if (threadIdx.x < kc && hist[threadIdx.x]) atomicAdd(&sizes[threadIdx.x], hist[threadIdx.x]);
}

// the means' bit counts, cnt[c][t] for bit t = 8 * byte + bit-in-byte: thread t owns column t of an LDS table, a tile of 256 descriptors at a
// time is staged in LDS; one atomic per non-zero counter per workgroup at the end
__global__ __launch_bounds__(kBlock) void k_bitcount(const ulonglong4* __restrict__ x, int n, const int* __restrict__ assoc, int kc,
                                                       int* __restrict__ cnt) {
  __shared__ uint32_t tile[kBlock * 8];
  __shared__ int ta[kBlock];
  __shared__ int acc[kMaxK * kBlock];
  const int t = threadIdx.x;
  for (int c = 0; c < kc; c++) acc[c * kBlock + t] = 0;
  const int ntiles = (n + kBlock - 1) / kBlock;
  for (int tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
    __syncthreads();
    const int i = tl * kBlock + t;
    const int m = min(kBlock, n - tl * kBlock);
    if (i < n) {
      const ulonglong4 v = x[i];
      uint32_t* d = tile + t * 8;
      d[0] = (uint32_t)v.x; d[1] = (uint32_t)(v.x >> 32); d[2] = (uint32_t)v.y; d[3] = (uint32_t)(v.y >> 32);
      d[4] = (uint32_t)v.z; d[5] = (uint32_t)(v.z >> 32); d[6] = (uint32_t)v.w; d[7] = (uint32_t)(v.w >> 32);
      ta[t] = assoc[i];
    }
    __syncthreads();
    const int wd = t >> 5, sh = t & 31;
    for (int j = 0; j < m; j++) acc[ta[j] * kBlock + t] += (tile[j * 8 + wd] >> sh) & 1u;
  }
  __syncthreads();
  for (int c = 0; c < kc; c++) {
    const int v = acc[c * kBlock + t];
    if (v) atomicAdd(&cnt[c * kBlock + t], v);
  }
}

// FORB::meanValue (FORB.cpp:28-77): bit set when its count >= n/2 + n%2 (one member: a copy, the same bits); an empty cluster keeps its
// previous centre (the reference releases it and then dereferences it).  Wave w's ballot is 64-bit word w of the descriptor.
__global__ __launch_bounds__(kBlock) void k_majority(const int* __restrict__ cnt, const int* __restrict__ sizes, int kc, uint64_t* __restrict__ cent,
                                                       int* __restrict__ empty) {
  const int t = threadIdx.x;
  for (int c = 0; c < kc; c++) {
    const int nc = sizes[c];
    if (nc == 0) {
      if (t == 0) empty[0] += 1;
      continue;
    }
    const int n2 = nc / 2 + nc % 2;
    const uint64_t m = __ballot(cnt[c * kBlock + t] >= n2);
    if ((t & 63) == 0) cent[c * 4 + (t >> 6)] = m;
  }
}

// stable partition, 1: per-block cluster counts, cluster-major (bc[c * nb + b]) so that one exclusive scan gives every destination base
__global__ __launch_bounds__(kBlock) void k_part_count(const int* __restrict__ assoc, int n, int kc, int nb, int* __restrict__ bc) {
  __shared__ int hist[kMaxK];
  if (threadIdx.x < kMaxK) hist[threadIdx.x] = 0;
  __syncthreads();
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) atomicAdd(&hist[assoc[i]], 1);
  __syncthreads();
  if (threadIdx.x < kc) bc[threadIdx.x * nb + blockIdx.x] = hist[threadIdx.x];
}

// 2: exclusive scan of m ints in place, one workgroup of 1024 (m <= 20 * 2^20 / 256)
__global__ __launch_bounds__(1024) void k_scan_excl(int* __restrict__ a, int m) {
  __shared__ int part[1024];
  const int t = threadIdx.x, per = (m + 1023) / 1024, b0 = min(m, t * per), b1 = min(m, b0 + per);
  int s = 0;
  for (int j = b0; j < b1; j++) s += a[j];
  part[t] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int v = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int run = part[t] - s;
  for (int j = b0; j < b1; j++) {
    const int v = a[j];
    a[j] = run;
    run += v;
  }
}

// 3: order-preserving scatter: rank inside the block from one ballot per cluster and wave
__global__ __launch_bounds__(kBlock) void k_part_scatter(const ulonglong4* __restrict__ x, int n, const int* __restrict__ assoc, int kc, int nb,
                                                           const int* __restrict__ bc, ulonglong4* __restrict__ y) {
  __shared__ int wc[kBlock / 64][kMaxK];
  const int i = blockIdx.x * kBlock + threadIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int a = i < n ? assoc[i] : -1;
  const uint64_t lt = (1ull << lane) - 1ull;
  int rank = 0;
  for (int c = 0; c < kc; c++) {
    const uint64_t m = __ballot(a == c);
    if (a == c) rank = __popcll(m & lt);
    if (lane == 0) wc[w][c] = __popcll(m);
  }
  __syncthreads();
  if (a >= 0) {
    for (int j = 0; j < w; j++) rank += wc[j][a];
    y[bc[a * nb + blockIdx.x] + rank] = x[i];
  }
}

#define TR_HIP(expr)                                                                                 \
  do {                                                                                               \
    const hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess) return fail(ORBX_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

int fail(int rc, const std::string& msg) {
  g_err = msg;
  return rc;
}

using Clock = std::chrono::steady_clock;
inline double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

struct Trainer {
  int k = 0, L = 0, thr = 0, max_it = 0;
  int64_t N = 0;
  GlibcRand rng;
  orbx_train_stats st{};
  // the tree, root = node 0 (TemplatedVocabulary::m_nodes order)
  std::vector<int32_t> parent;
  std::vector<uint64_t> node_desc;   // 4 words per node
  // host working set
  std::vector<uint64_t> hbuf[2];
  std::vector<int32_t> md, assoc;
  // device working set (allocated when some node is large enough)
  bool dev = false;
  ulonglong4* dbuf[2] = {nullptr, nullptr};
  int *d_md = nullptr, *d_assoc = nullptr, *d_bc = nullptr, *d_cnt = nullptr, *d_small = nullptr;   // d_small: sizes[20], changed, empty
  long long* d_bsum = nullptr;
  ulonglong4* d_cent = nullptr;
  unsigned long long* d_total = nullptr;
  int* h_pin = nullptr;   // pinned: total (2 ints), changed, sizes[20], empty
  uint64_t* h_cent = nullptr;
  hipStream_t s = nullptr;

  explicit Trainer(uint32_t seed) : rng(seed) {}
  ~Trainer() {
    for (auto* p : {(void*)dbuf[0], (void*)dbuf[1], (void*)d_md, (void*)d_assoc, (void*)d_bc, (void*)d_cnt, (void*)d_small, (void*)d_bsum,
                    (void*)d_cent, (void*)d_total})
      if (p) (void)hipFree(p);
    if (h_pin) (void)hipHostFree(h_pin);
    if (h_cent) (void)hipHostFree(h_cent);
    if (s) (void)hipStreamDestroy(s);
  }

  int dev_init() {
    const size_t n = (size_t)N, nb = (n + kBlock - 1) / kBlock;
    TR_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    for (int b = 0; b < 2; b++) TR_HIP(hipMalloc((void**)&dbuf[b], n * 32));
    TR_HIP(hipMalloc((void**)&d_md, n * 4));
    TR_HIP(hipMalloc((void**)&d_assoc, n * 4));
    TR_HIP(hipMalloc((void**)&d_bc, nb * kMaxK * 4));
    TR_HIP(hipMalloc((void**)&d_cnt, kMaxK * kBlock * 4));
    TR_HIP(hipMalloc((void**)&d_small, 64 * 4));
    TR_HIP(hipMalloc((void**)&d_bsum, nb * 8));
    TR_HIP(hipMalloc((void**)&d_cent, kMaxK * 32));
    TR_HIP(hipMalloc((void**)&d_total, 8));
    TR_HIP(hipHostMalloc((void**)&h_pin, 64 * 4));
    TR_HIP(hipHostMalloc((void**)&h_cent, kMaxK * 32));
    TR_HIP(hipMemcpyAsync(dbuf[0], hbuf[0].data(), n * 32, hipMemcpyHostToDevice, s));
    TR_HIP(hipStreamSynchronize(s));
    dev = true;
    return ORBX_OK;
  }

  // ---- host k-means of one node: hbuf[src] range [off, off + n) -> centres, sizes, hbuf[src ^ 1] partitioned -------------------------
  int host_kmeans(int src, int64_t off, int n, std::vector<uint64_t>& cent, std::vector<int>& sizes) {
    const uint64_t* X = hbuf[src].data() + off * 4;
    int32_t* dist = md.data() + off;
    int32_t* as = assoc.data() + off;
    // initiateClustersKMpp (:833-915)
    cent.clear();
    int ifeat = rng.random_int(0, n - 1);
    cent.insert(cent.end(), X + 4 * ifeat, X + 4 * ifeat + 4);
    for (int i = 0; i < n; i++) dist[i] = hamming4(X + 4 * i, X + 4 * ifeat);
    while ((int)cent.size() / 4 < k) {
      int64_t sum = 0;
      for (int i = 0; i < n; i++) sum += dist[i];
      if (sum == 0) break;
      double cutd;
      do cutd = rng.random_value(0, (double)sum); while (cutd == 0.0);
      const int64_t cut = (int64_t)std::ceil(cutd);
      int64_t run = 0;
      ifeat = n - 1;
      for (int i = 0; i < n; i++) {
        run += dist[i];
        if (run >= cut) { ifeat = i; break; }
      }
      cent.insert(cent.end(), X + 4 * ifeat, X + 4 * ifeat + 4);
      if ((int)cent.size() / 4 < k)
        for (int i = 0; i < n; i++) dist[i] = std::min(dist[i], hamming4(X + 4 * i, X + 4 * ifeat));
    }
    const int kc = (int)cent.size() / 4;
    sizes.assign(kc, 0);
    auto assign = [&](bool first) {
      bool changed = false;
      std::fill(sizes.begin(), sizes.end(), 0);
      for (int i = 0; i < n; i++) {
        const uint64_t* x = X + 4 * i;
        int best = hamming4(x, cent.data()), bi = 0;
        for (int c = 1; c < kc; c++) {
          const int d = hamming4(x, cent.data() + 4 * c);
          if (d < best) { best = d; bi = c; }
        }
        if (!first && as[i] != bi) changed = true;
        as[i] = bi;
        sizes[bi]++;
      }
      return changed;
    };
    assign(true);
    int it = 1;
    uint64_t lanes[kMaxK][32];
    int32_t cnt[kMaxK][256];
    uint8_t since[kMaxK];
    for (;;) {
      if (it >= max_it) return fail(ORBX_E_NOCONVERGE, "k-means did not converge within max_iterations (" + std::to_string(max_it) + ")");
      // FORB::meanValue of every group
      std::memset(lanes, 0, sizeof(uint64_t) * 32 * kc);
      std::memset(cnt, 0, sizeof(int32_t) * 256 * kc);
      std::memset(since, 0, kc);
      auto flush = [&](int c) {
        for (int j = 0; j < 32; j++) {
          const uint64_t v = lanes[c][j];
          for (int p = 0; p < 8; p++) cnt[c][8 * j + p] += (int)((v >> (8 * p)) & 0xff);
          lanes[c][j] = 0;
        }
        since[c] = 0;
      };
      for (int i = 0; i < n; i++) {
        const int c = as[i];
        const uint8_t* b = (const uint8_t*)(X + 4 * i);
        for (int j = 0; j < 32; j++) lanes[c][j] += kSpread.t[b[j]];
        if (++since[c] == 255) flush(c);
      }
      for (int c = 0; c < kc; c++) {
        if (sizes[c] == 0) { st.empty_clusters++; continue; }   // departure: the previous centre stays
        flush(c);
        const int n2 = sizes[c] / 2 + sizes[c] % 2;
        uint8_t* m = (uint8_t*)(cent.data() + 4 * c);
        for (int j = 0; j < 32; j++) {
          uint8_t v = 0;
          for (int p = 0; p < 8; p++) v |= (uint8_t)((cnt[c][8 * j + p] >= n2) << p);
          m[j] = v;
        }
      }
      it++;
      if (!assign(false)) break;
    }
    st.iterations += it;
    // stable partition into the other buffer
    uint64_t* Y = hbuf[src ^ 1].data() + off * 4;
    int pos[kMaxK];
    for (int c = 0, run = 0; c < kc; c++) { pos[c] = run; run += sizes[c]; }
    for (int i = 0; i < n; i++) std::memcpy(Y + 4 * (pos[as[i]]++), X + 4 * i, 32);
    return ORBX_OK;
  }

  int dev_read(void* dst, const void* src, size_t bytes) {
    TR_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s));
    TR_HIP(hipStreamSynchronize(s));
    return ORBX_OK;
  }

  // ---- device k-means of one node: dbuf[src] range -> centres, sizes, dbuf[src ^ 1] partitioned ------------------------------------
  int dev_kmeans(int src, int64_t off, int n, std::vector<uint64_t>& cent, std::vector<int>& sizes) {
    const ulonglong4* X = dbuf[src] + off;
    ulonglong4* Y = dbuf[src ^ 1] + off;
    const int nb = (n + kBlock - 1) / kBlock;
    int* d_sizes = d_small;
    int* d_changed = d_small + kMaxK;
    int* d_empty = d_small + kMaxK + 1;
    int rc;
    TR_HIP(hipMemsetAsync(d_small, 0, 64 * 4, s));
    int ifeat = rng.random_int(0, n - 1);
    TR_HIP(hipMemcpyAsync(d_cent, X + ifeat, 32, hipMemcpyDeviceToDevice, s));
    TR_HIP(hipMemsetAsync(d_total, 0, 8, s));
    hipLaunchKernelGGL(k_seed_dist, dim3(nb), dim3(kBlock), 0, s, X, n, (const uint64_t*)d_cent, 1, d_md, d_bsum, d_total);
    int kc = 1;
    while (kc < k) {
      if ((rc = dev_read(h_pin, d_total, 8)) != ORBX_OK) return rc;
      int64_t sum;
      std::memcpy(&sum, h_pin, 8);
      if (sum == 0) break;
      double cutd;
      do cutd = rng.random_value(0, (double)sum); while (cutd == 0.0);
      hipLaunchKernelGGL(k_seed_select, dim3(1), dim3(kBlock), 0, s, X, n, d_md, d_bsum, nb, (long long)std::ceil(cutd), d_cent, kc);
      kc++;
      if (kc < k) {
        TR_HIP(hipMemsetAsync(d_total, 0, 8, s));
        hipLaunchKernelGGL(k_seed_dist, dim3(nb), dim3(kBlock), 0, s, X, n, (const uint64_t*)(d_cent + kc - 1), 0, d_md, d_bsum, d_total);
      }
    }
    TR_HIP(hipGetLastError());
    const int gb = std::min(nb, 1024);
    hipLaunchKernelGGL(k_assign, dim3(nb), dim3(kBlock), 0, s, X, n, d_cent, kc, 1, d_assoc, d_changed, d_sizes);
    int it = 1;
    for (;;) {
      if (it >= max_it) return fail(ORBX_E_NOCONVERGE, "k-means did not converge within max_iterations (" + std::to_string(max_it) + ")");
      TR_HIP(hipMemsetAsync(d_cnt, 0, kMaxK * kBlock * 4, s));
      hipLaunchKernelGGL(k_bitcount, dim3(gb), dim3(kBlock), 0, s, X, n, d_assoc, kc, d_cnt);
      hipLaunchKernelGGL(k_majority, dim3(1), dim3(kBlock), 0, s, d_cnt, d_sizes, kc, (uint64_t*)d_cent, d_empty);
      TR_HIP(hipMemsetAsync(d_small, 0, (kMaxK + 1) * 4, s));   // sizes + changed (not the empty counter)
      hipLaunchKernelGGL(k_assign, dim3(nb), dim3(kBlock), 0, s, X, n, d_cent, kc, 0, d_assoc, d_changed, d_sizes);
      TR_HIP(hipGetLastError());
      it++;
      if ((rc = dev_read(h_pin, d_small, (kMaxK + 2) * 4)) != ORBX_OK) return rc;
      if (!h_pin[kMaxK]) break;
    }
    st.iterations += it;
    st.empty_clusters += h_pin[kMaxK + 1];
    sizes.assign(h_pin, h_pin + kc);
    hipLaunchKernelGGL(k_part_count, dim3(nb), dim3(kBlock), 0, s, d_assoc, n, kc, nb, d_bc);
    hipLaunchKernelGGL(k_scan_excl, dim3(1), dim3(1024), 0, s, d_bc, kc * nb);
    hipLaunchKernelGGL(k_part_scatter, dim3(nb), dim3(kBlock), 0, s, X, n, d_assoc, kc, nb, d_bc, Y);
    TR_HIP(hipGetLastError());
    if ((rc = dev_read(h_cent, d_cent, (size_t)kc * 32)) != ORBX_OK) return rc;
    cent.assign(h_cent, h_cent + 4 * kc);
    return ORBX_OK;
  }

  // HKmeansStep(parent_id, descriptors, current_level) (:642-822) on the range [off, off + n) of buffer (level - 1) & 1
  int step(int32_t pid, int64_t off, int n, int level, bool on_dev) {
    if (n == 0) return ORBX_OK;
    const int src = (level - 1) & 1;
    std::vector<uint64_t> cent;
    std::vector<int> sizes;
    int rc = ORBX_OK;
    bool children_dev = false;
    if (n <= k) {   // one cluster per descriptor, duplicates included; no draw
      const uint64_t* X = hbuf[src].data() + off * 4;
      cent.assign(X, X + 4 * (size_t)n);
      sizes.assign(n, 1);
    } else if (on_dev) {
      const auto t0 = Clock::now();
      rc = dev_kmeans(src, off, n, cent, sizes);
      st.device_nodes++;
      st.ms_device += ms_since(t0);
      children_dev = true;
    } else {
      const auto t0 = Clock::now();
      rc = host_kmeans(src, off, n, cent, sizes);
      st.host_nodes++;
      st.ms_host += ms_since(t0);
    }
    if (rc != ORBX_OK) return rc;
    const int kc = (int)sizes.size();
    const int32_t first = (int32_t)parent.size();
    for (int c = 0; c < kc; c++) {
      parent.push_back(pid);
      node_desc.insert(node_desc.end(), cent.begin() + 4 * c, cent.begin() + 4 * c + 4);
    }
    if (level >= L) return ORBX_OK;
    if (children_dev) {   // children that continue on the host need their range there
      bool any_host = false;
      for (int c = 0; c < kc; c++) any_host |= sizes[c] > 1 && !(sizes[c] >= thr && sizes[c] > k);
      if (any_host) {
        const auto t0 = Clock::now();
        if ((rc = dev_read(hbuf[src ^ 1].data() + off * 4, dbuf[src ^ 1] + off, (size_t)n * 32)) != ORBX_OK) return rc;
        st.ms_device += ms_since(t0);
      }
    }
    int64_t o = off;
    for (int c = 0; c < kc; c++) {
      if (sizes[c] > 1) {
        const bool d = children_dev && sizes[c] >= thr && sizes[c] > k;
        if ((rc = step(first + c, o, sizes[c], level + 1, d)) != ORBX_OK) return rc;
      }
      o += sizes[c];
    }
    return ORBX_OK;
  }
};

}  // namespace

extern "C" {

const char* orbx_train_last_error(void) { return g_err.c_str(); }

int orbx_train_glibc_rand(uint32_t seed, int n, int32_t* out) {
  if (n < 0 || (n > 0 && !out)) return ORBX_E_INVALID;
  GlibcRand r(seed);
  for (int i = 0; i < n; i++) out[i] = r.next();
  return ORBX_OK;
}

int orbx_train_vocabulary(orbx_ctx* ctx, const uint8_t* desc, const int64_t* doc_offsets, int ndocs, const orbx_train_params* p,
                          orbx_voc** out, orbx_train_stats* stats) {
  g_err.clear();
  if (!ctx || !doc_offsets || ndocs < 0 || !p || !out) return fail(ORBX_E_INVALID, "null argument");
  *out = nullptr;
  if (p->k < 2 || p->k > kMaxK || p->L < 1 || p->L > 10 || p->weighting < 0 || p->weighting > 3 || p->scoring < 0 || p->scoring > 5 ||
      p->max_iterations < 0)
    return fail(ORBX_E_INVALID, "k must be 2..20, L 1..10, weighting 0..3, scoring 0..5");
  if (doc_offsets[0] != 0) return fail(ORBX_E_INVALID, "doc_offsets[0] must be 0");
  for (int d = 0; d < ndocs; d++)
    if (doc_offsets[d + 1] < doc_offsets[d]) return fail(ORBX_E_INVALID, "doc_offsets must not decrease");
  const int64_t N = doc_offsets[ndocs];
  if (N > (1ll << 27)) return fail(ORBX_E_CAPACITY, "more than 2^27 training descriptors");
  if (N > 0 && !desc) return fail(ORBX_E_INVALID, "null descriptors");
  Trainer T(p->seed);
  T.k = p->k; T.L = p->L; T.N = N;
  T.thr = p->device_min_node < 0 ? ORBX_TRAIN_DEVICE_MIN_NODE : std::max(p->device_min_node, p->k + 1);
  T.max_it = p->max_iterations ? p->max_iterations : ORBX_TRAIN_MAX_ITERATIONS;
  T.parent.assign(1, 0);   // the root
  T.node_desc.assign(4, 0);
  T.hbuf[0].resize((size_t)N * 4);
  T.hbuf[1].resize((size_t)N * 4);
  T.md.resize((size_t)N);
  T.assoc.resize((size_t)N);
  if (N) std::memcpy(T.hbuf[0].data(), desc, (size_t)N * 32);
  int rc;
  const bool root_dev = N > T.k && N >= T.thr;
  if (root_dev && (rc = T.dev_init()) != ORBX_OK) return rc;
  if ((rc = T.step(0, 0, (int)N, 1, root_dev)) != ORBX_OK) return rc;
  // createWords (:918-940): leaves in node-id order; setNodeWeights (:943-995)
  const int nn = (int)T.parent.size();
  std::vector<uint8_t> leaf(nn, 1), ndesc((size_t)nn * 32);
  for (int i = 1; i < nn; i++) leaf[T.parent[i]] = 0;
  std::memcpy(ndesc.data(), T.node_desc.data(), ndesc.size());
  std::vector<double> weight(nn, 0.0);
  std::vector<int> word_of(nn, -1);
  int nwords = 0;
  for (int i = 1; i < nn; i++)
    if (leaf[i]) word_of[i] = nwords++;
  auto t0 = Clock::now();
  orbx_voc* v = nullptr;
  if (nn <= 1) return fail(ORBX_E_INVALID, "no training descriptors");
  const bool idf = p->weighting == 0 || p->weighting == 2;
  if (!idf) {
    for (int i = 1; i < nn; i++)
      if (leaf[i]) weight[i] = 1;
  } else {
    // the tree first with zero weights: orbx_bow_transform (the product's device descent = transform(feature, word_id), :363) sends every
    // training descriptor down; Ni = documents per word
    if ((rc = orbx_voc_create(ctx, T.k, T.L, p->scoring, p->weighting, nn - 1, T.parent.data() + 1, leaf.data() + 1, ndesc.data() + 32,
                              weight.data() + 1, &v)) != ORBX_OK)
      return fail(rc, std::string("orbx_voc_create: ") + orbx_last_error(ctx));
    T.st.ms_create += ms_since(t0);
    t0 = Clock::now();
    std::vector<uint32_t> word((size_t)std::max<int64_t>(N, 1)), node((size_t)std::max<int64_t>(N, 1));
    std::vector<double> wt((size_t)std::max<int64_t>(N, 1));
    const int64_t chunk = 1 << 16;
    for (int64_t a = 0; a < N; a += chunk) {
      const int m = (int)std::min(chunk, N - a);
      if ((rc = orbx_bow_transform(v, desc + a * 32, m, 0, word.data() + a, wt.data() + a, node.data() + a)) != ORBX_OK) {
        const std::string e = orbx_last_error(ctx);
        orbx_voc_destroy(v);
        return fail(rc, "orbx_bow_transform: " + e);
      }
    }
    orbx_voc_destroy(v);
    v = nullptr;
    std::vector<uint32_t> Ni(nwords, 0);
    std::vector<int> counted(nwords, -1);
    for (int d = 0; d < ndocs; d++)
      for (int64_t i = doc_offsets[d]; i < doc_offsets[d + 1]; i++) {
        const uint32_t w = word[i];
        if (w >= (uint32_t)nwords) return fail(ORBX_E_DEVICE, "descent returned a word id out of range");
        if (counted[w] != d) { Ni[w]++; counted[w] = d; }
      }
    for (int i = 1; i < nn; i++)
      if (leaf[i] && Ni[word_of[i]] > 0) weight[i] = std::log((double)ndocs / (double)Ni[word_of[i]]);
    T.st.ms_weights += ms_since(t0);
    t0 = Clock::now();
  }
  if ((rc = orbx_voc_create(ctx, T.k, T.L, p->scoring, p->weighting, nn - 1, T.parent.data() + 1, leaf.data() + 1, ndesc.data() + 32,
                            weight.data() + 1, &v)) != ORBX_OK)
    return fail(rc, std::string("orbx_voc_create: ") + orbx_last_error(ctx));
  T.st.ms_create += ms_since(t0);
  *out = v;
  if (stats) *stats = T.st;
  return ORBX_OK;
}

}  // extern "C"
