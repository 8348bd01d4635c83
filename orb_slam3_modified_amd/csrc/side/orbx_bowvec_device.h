// Device helpers of the kernels that intersect two batches of BowVectors a wave per (query, database) pair (csrc/score/orbx_score.hip,
// csrc/place/orbx_place.hip): where a vector lies, the query's image in LDS, and the search of one id in it.  Below csrc/, outside
// kernels_hash().
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace orbx {
namespace side {

// one side of the matrix: fixed stride with counts (n), or compact CSR (ptr)
struct Side { const uint32_t* ids; const double* vals; const int32_t* n; const int32_t* ptr; int stride; };
__device__ __forceinline__ void side_row(const Side& s, int i, size_t* start, int* n) {
  if (s.ptr) { *start = (size_t)s.ptr[i]; *n = s.ptr[i + 1] - s.ptr[i]; }      // ascending from >= 0: checked on the host
  else { *start = (size_t)i * s.stride; *n = min(max(s.n[i], 0), s.stride); }
}

// A row of qn entries (gi, gv) staged by the whole workgroup into s_id (room for qn + 4) and s_v (room for qn + 2), both 16-byte aligned,
// by 16-byte loads: the LDS image keeps the row's offset inside its 16-byte line, so that an aligned global chunk is an aligned LDS chunk;
// the row's ragged ends go entry by entry.  Entry j lies at s_id[j + *mi] and s_v[j + *mv].  The caller's barrier follows.
__device__ __forceinline__ void stage_row(const uint32_t* gi, const double* gv, int qn, uint32_t* s_id, double* s_v, int tid, int nthreads,
                                          int* mi, int* mv) {
  const int oi = (int)(((uintptr_t)gi >> 2) & 3), ov = (int)(((uintptr_t)gv >> 3) & 1);
  // chunk c of an image holds its elements 4c .. 4c + 3 (2c, 2c + 1): a chunk that lies inside the row is one 16-byte load
  const uint4* const gi4 = (const uint4*)(gi - oi);
  for (int c = tid; 4 * c < oi + qn; c += nthreads) {
    if (4 * c >= oi && 4 * c + 4 <= oi + qn) ((uint4*)s_id)[c] = gi4[c];
    else
      for (int e = max(4 * c, oi); e < min(4 * c + 4, oi + qn); e++) s_id[e] = gi[e - oi];
  }
  const double2* const gv2 = (const double2*)(gv - ov);
  for (int c = tid; 2 * c < ov + qn; c += nthreads) {
    if (2 * c >= ov && 2 * c + 2 <= ov + qn) ((double2*)s_v)[c] = gv2[c];
    else
      for (int e = max(2 * c, ov); e < min(2 * c + 2, ov + qn); e++) s_v[e] = gv[e - ov];
  }
  *mi = oi; *mv = ov;
}

// lower_bound: the first of the qn ascending ids that is not below `id`
__device__ __forceinline__ int first_not_below(const uint32_t* qi, int qn, uint32_t id) {
  int lo = 0, len = qn;
  while (len > 0) {
    const int half = len >> 1;
    if (qi[lo + half] < id) { lo += half + 1; len -= half + 1; } else len = half;
  }
  return lo;
}

}  // namespace side
}  // namespace orbx
