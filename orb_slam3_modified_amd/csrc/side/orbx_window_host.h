// The host side the four chained projection matchers share (liborbx_localmatch.so, liborbx_lastmatch.so, liborbx_projmatch.so,
// liborbx_rigmatch.so): the handle, the argument checks of both forms, the LDS-or-scratch plan, the level table, the tail of a device form
// (launch) and a host form's one-camera side in the handle's io block.  Host code of a .hip source only, beside orbx_handle.h.
#pragma once
#include <algorithm>
#include <climits>
#include <string>

#include "orbx_handle.h"
#include "orbx_window_device.h"

namespace orbx {
namespace side {
namespace win {

struct WindowHandle : Handle {     // scratch: per workgroup the global path's arrays
  int lds_limit = kLdsMax;         // the library's ORBX_*_LDS at create
};

// a create's init: the limit from `env`, the LDS instantiation allowed its largest block
inline const char* open_window(WindowHandle* m, const char* env, const void* lds_kernel) {
  m->lds_limit = env_int(env, 0, kLdsMax, kLdsMax);
  return allow_lds(lds_kernel, kLdsMax);
}

template <class S>                 // orbx_*_side: d_uright, where a side has one, may be null
const char* side_problem(const S* s) {
  if (!s) return "null side";
  if (s->nframes < 1 || s->capacity < 1) return "nframes and capacity must be at least 1";
  if (s->capacity > kMaxCap) return "capacity above 32768";
  if (!s->d_kps || !s->d_desc || !s->d_counts || !s->d_bounds) return "null buffer in the side";
  if ((long long)s->nframes * s->capacity > (long long)INT_MAX) return "nframes * capacity exceeds INT_MAX";
  return nullptr;
}

// What both forms check before anything is copied or launched.  `inputs` / `outputs`: all of the library's own pointers are there, named
// in the message by `in_names` / `out_names`; `own`: a problem of the library's own arguments, reported in its place.
template <class S>
int check_call(Handle* m, const char* who, const S* side, bool inputs, const char* in_names, bool outputs, const char* out_names, int nitems,
               int mcap, int npoints, const float* sf, int nlevels, const char* own = nullptr) {
  if (const char* e = side_problem(side)) return fail(m, ORBX_E_INVALID, std::string(who) + e);
  if (!inputs) return fail(m, ORBX_E_INVALID, std::string(who) + "null " + in_names);
  if (!outputs) return fail(m, ORBX_E_INVALID, std::string(who) + "null " + out_names);
  if (nitems < 1 || mcap < 1 || npoints < 1) return fail(m, ORBX_E_INVALID, std::string(who) + "nitems, mcap and npoints must be at least 1");
  if (!sf || nlevels < 1 || nlevels > kMaxLevels)
    return fail(m, ORBX_E_INVALID, std::string(who) + "scale_factors and nlevels in 1 .. 16 are needed (nlevels = " + std::to_string(nlevels) + ")");
  if (own) return fail(m, ORBX_E_INVALID, std::string(who) + own);
  if ((long long)mcap * side->capacity > (long long)INT_MAX || (long long)nitems * std::max(mcap, side->capacity) > (long long)INT_MAX)
    return fail(m, ORBX_E_INVALID, std::string(who) + "mcap * capacity or nitems * max(mcap, capacity) exceeds INT_MAX");
  return ORBX_OK;
}

// the bitonic sort's size for a grid of up to cap keypoints
inline int sort_size(int cap) {
  int p2 = 2;
  while (p2 < cap) p2 <<= 1;
  return p2;
}

// where the kernel keeps its arrays, from the layout's sizes on both paths; `longest`: one point's longest list(s), in candidates
inline int plan(WindowHandle* m, size_t fixed_lds, size_t fixed_global, int longest, int nitems, Paths* path) {
  return plan_paths(m, m->lds_limit, fixed_lds, fixed_global, longest, nitems, {kMaxBlocks, kGlobalBlocks, kGlobalRoom}, path);
}
// one camera: the sort's size too; one point's longest list is cap candidates
inline int plan(WindowHandle* m, int cap, int mcap, int nitems, int* p2, Paths* path) {
  *p2 = sort_size(cap);
  return plan(m, layout(cap, mcap, *p2, true).fixed, layout(cap, mcap, *p2, false).fixed, cap, nitems, path);
}

inline void fill_levels(float (&dst)[kMaxLevels], const float* sf, int nlevels) {
  for (int l = 0; l < kMaxLevels; l++) dst[l] = l < nlevels ? sf[l] : 0.0f;
}

// The tail of a device form: the plan's scratch and room into the kernel's arguments (scratch, scratch_stride, room), the caller's stream or
// the handle's, after the handle's previous call, the kernel's LDS or global instantiation, the call's record.
template <class A>
int launch(WindowHandle* m, const Paths& path, A& g, void (*lds_kernel)(A), void (*global_kernel)(A), void* stream) {
  g.scratch = path.in_lds ? nullptr : m->scratch.p; g.scratch_stride = path.scratch_stride; g.room = path.room;
  hipStream_t st = stream ? (hipStream_t)stream : m->st;
  const int rc = wait_previous(m, st);
  if (rc != ORBX_OK) return rc;
  if (path.in_lds) hipLaunchKernelGGL(lds_kernel, dim3((unsigned)path.blocks), dim3(kThreads), path.lds_bytes, st, g);
  else hipLaunchKernelGGL(global_kernel, dim3((unsigned)path.blocks), dim3(kThreads), 0, st, g);
  return record_call(m, st);
}

// A host form's one-camera side (orbx_localmatch_side, orbx_lastmatch_side, orbx_projmatch_side) in the handle's io block.  `uright`: the
// side's d_uright member where it has one; a null array stays null on the device side.
struct StagedSide { size_t kps, desc, counts, uright, bounds; };
template <class S>
StagedSide stage_side(Stager& io, const S* s, const float* S::*uright = nullptr) {
  const size_t nf = (size_t)s->nframes, nk = nf * s->capacity;
  StagedSide o;
  o.kps = io.in(s->d_kps, nk * sizeof(orbx_keypoint)); o.desc = io.in(s->d_desc, nk * 32); o.counts = io.in(s->d_counts, nf * 8);
  o.uright = uright && s->*uright ? io.in(s->*uright, nk * 4) : 0; o.bounds = io.in(s->d_bounds, nf * 16);
  return o;
}
template <class S>
S device_side(uint8_t* d, const StagedSide& o, const S* s, const float* S::*uright = nullptr) {
  S ds = *s;
  ds.d_kps = (const orbx_keypoint*)(d + o.kps); ds.d_desc = d + o.desc; ds.d_counts = (const int32_t*)(d + o.counts);
  ds.d_bounds = (const float*)(d + o.bounds);
  if (uright && s->*uright) ds.*uright = (const float*)(d + o.uright);
  return ds;
}

}  // namespace win
}  // namespace side
}  // namespace orbx
