// The host side the four pair matchers share (liborbx_match.so, liborbx_rigbow.so, liborbx_trimatch.so, liborbx_initmatch.so): the handle,
// the checks of both forms that are every library's, a host form's two sides in the handle's io block and the tail of a device form
// (launch).  Host code of a .hip source only, beside orbx_handle.h; the device half is orbx_pair_device.h.  No kernel is stated here: each
// library keeps its own.
#pragma once
#include <algorithm>
#include <climits>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "orbx_handle.h"

namespace orbx {
namespace side {
namespace pair {

constexpr int kLdsMax = 152 * 1024;       // dynamic LDS of one workgroup (160 KiB per CU, the kernels' static part is below 4 KiB)
constexpr int kMaxBlocks = 1024;          // workgroups of one launch: on the global path each owns one slice of the scratch
constexpr int kWaveNode = 64;

struct PairHandle : Handle {       // scratch: per workgroup the global path's arrays
  int lds_limit = kLdsMax;         // the library's ORBX_*_LDS at create
  int wave_node = kWaveNode;       // the library's ORBX_*_WAVE_NODE at create, where it has one
};

// a create's init: the limits from the library's variables (`wave_env` null: it has none), the LDS instantiation allowed its largest block
inline const char* open_pair(PairHandle* m, const char* lds_env, const char* wave_env, const void* lds_kernel) {
  m->lds_limit = env_int(lds_env, 0, kLdsMax, kLdsMax);
  if (wave_env) m->wave_node = env_int(wave_env, 0, kWaveNode, kWaveNode);
  return allow_lds(lds_kernel, kLdsMax);
}

// FV: the side carries a FeatureVector (d_fv_node, d_fv_ptr, d_fv_feat, d_fv_n); `max_cap`: the library's ceiling (0: none), `above`
// its message.  A side's optional arrays may be null.
template <bool FV, class S>
const char* side_problem(const S* s, int max_cap, const char* above) {
  if (!s) return "null side";
  if (s->nframes < 1 || s->capacity < 1) return "nframes and capacity must be at least 1";
  if (max_cap && s->capacity > max_cap) return above;
  bool all = s->d_kps && s->d_desc && s->d_counts;
  if constexpr (FV) all = all && s->d_fv_node && s->d_fv_ptr && s->d_fv_feat && s->d_fv_n;
  return all ? nullptr : "null buffer in a side";
}

// What both forms check before anything is copied or launched, in three steps between which a library puts the checks that are its own.
// First the two sides and the library's other pointers (`args`: the needed ones are all there; `names` names them in the message),
template <bool FV, class S>
int check_sides(Handle* m, const char* who, const S* a, const S* b, int max_cap, const char* above, bool args, const char* names) {
  for (const S* s : {a, b})
    if (const char* e = side_problem<FV>(s, max_cap, above)) return fail(m, ORBX_E_INVALID, std::string(who) + e);
  return args ? ORBX_OK : fail(m, ORBX_E_INVALID, std::string(who) + "null " + names);
}
// then the number of pairs,
inline int check_npairs(Handle* m, const char* who, int npairs) {
  return npairs >= 1 ? ORBX_OK : fail(m, ORBX_E_INVALID, std::string(who) + "npairs = " + std::to_string(npairs) + " (at least 1)");
}
// last the products an int must hold: npairs * `row` (the library's widest row of results for one pair, named by `product`) and every side's
// longest array, which with a FeatureVector is fv_ptr's nframes * (capacity + 1).
template <bool FV, class S>
int check_sizes(Handle* m, const char* who, const S* a, const S* b, int npairs, long long row, const char* product) {
  const int more = FV ? 1 : 0;
  if (npairs * row > (long long)INT_MAX || (long long)a->nframes * (a->capacity + more) > (long long)INT_MAX ||
      (long long)b->nframes * (b->capacity + more) > (long long)INT_MAX)
    return fail(m, ORBX_E_INVALID, std::string(who) + product + " or nframes * capacity exceeds INT_MAX");
  return ORBX_OK;
}

// One array of a side for a host form: where its pointer lies in the orbx_*_side, its bytes for each frame and for each of the
// nframes * capacity keypoints, and whether it may be null (then it stays null on the device side and nothing is copied).
struct Array { size_t member, per_frame, per_keypoint; bool optional; };
template <class S>
const void* get(const S* s, const Array& f) {
  const void* p;
  std::memcpy(&p, (const uint8_t*)s + f.member, sizeof(p));
  return p;
}
// a side's arrays in the order a host form declares them: keypoints, descriptors, counts, the FeatureVector where it has one, then its `own`
template <bool FV, class S>
std::vector<Array> side_arrays(std::initializer_list<Array> own = {}) {
  std::vector<Array> v = {{offsetof(S, d_kps), 0, sizeof(orbx_keypoint), false}, {offsetof(S, d_desc), 0, 32, false}, {offsetof(S, d_counts), 8, 0, false}};
  if constexpr (FV)
    v.insert(v.end(), {{offsetof(S, d_fv_node), 0, 4, false}, {offsetof(S, d_fv_ptr), 4, 4, false}, {offsetof(S, d_fv_feat), 0, 4, false},
                       {offsetof(S, d_fv_n), 4, 0, false}});
  v.insert(v.end(), own);
  return v;
}

// A host form's two sides in the handle's io block: stage_sides declares their arrays as inputs (one batch on both sides -- a == b, or
// structs that compare equal -- is staged once), device_sides gives the two orbx_*_side of the copies at `d` after the upload.
struct StagedSides { std::vector<size_t> off[2]; };
template <class S>
StagedSides stage_sides(Stager& io, const S* a, const S* b, const std::vector<Array>& arrays) {
  const bool same = a == b || std::memcmp(a, b, sizeof(S)) == 0;
  const S* sides[2] = {a, b};
  StagedSides o;
  for (int s = 0; s < (same ? 1 : 2); s++) {
    const size_t nf = (size_t)sides[s]->nframes, nk = nf * sides[s]->capacity;
    for (const Array& f : arrays) {
      const void* p = get(sides[s], f);
      o.off[s].push_back(p || !f.optional ? io.in(p, nf * f.per_frame + nk * f.per_keypoint) : 0);
    }
  }
  if (same) o.off[1] = o.off[0];
  return o;
}
template <class S>
void device_sides(uint8_t* d, const StagedSides& o, const S* a, const S* b, const std::vector<Array>& arrays, S (&ds)[2]) {
  const S* sides[2] = {a, b};
  for (int s = 0; s < 2; s++) {
    ds[s] = *sides[s];
    for (size_t k = 0; k < arrays.size(); k++) {
      const void* p = d + o.off[s][k];
      if (get(sides[s], arrays[k])) std::memcpy((uint8_t*)&ds[s] + arrays[k].member, &p, sizeof(p));
    }
  }
}

// The tail of a device form: on the global path `scratch_stride` bytes of the handle's scratch for each of the `blocks` workgroups (grown
// here unless a plan already has) into the kernel's arguments (scratch, scratch_stride), the caller's stream or the handle's, after the
// handle's previous call, the kernel's LDS or global instantiation, the call's record.
template <class A>
int launch(PairHandle* m, bool in_lds, size_t lds_bytes, size_t scratch_stride, int blocks, int threads, A& g, void (*lds_kernel)(A),
           void (*global_kernel)(A), void* stream) {
  int rc = in_lds ? ORBX_OK : grow(m, &m->scratch, scratch_stride * blocks);
  if (rc != ORBX_OK) return rc;
  g.scratch = in_lds ? nullptr : m->scratch.p; g.scratch_stride = in_lds ? 0 : scratch_stride;
  hipStream_t st = stream ? (hipStream_t)stream : m->st;
  if ((rc = wait_previous(m, st)) != ORBX_OK) return rc;
  if (in_lds) hipLaunchKernelGGL(lds_kernel, dim3((unsigned)blocks), dim3((unsigned)threads), lds_bytes, st, g);
  else hipLaunchKernelGGL(global_kernel, dim3((unsigned)blocks), dim3((unsigned)threads), 0, st, g);
  return record_call(m, st);
}

}  // namespace pair
}  // namespace side
}  // namespace orbx
