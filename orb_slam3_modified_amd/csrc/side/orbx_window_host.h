// The host side the three chained projection matchers share (liborbx_localmatch.so, liborbx_lastmatch.so, liborbx_projmatch.so): the
// handle, the argument checks of both forms, the LDS-or-scratch plan and the level table.  Host code only, beside orbx_handle.h.
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

// the sort's size and where the kernel keeps its arrays; one point's longest list is cap candidates
inline int plan(WindowHandle* m, int cap, int mcap, int nitems, int* p2, Paths* path) {
  *p2 = 2;
  while (*p2 < cap) *p2 <<= 1;
  return plan_paths(m, m->lds_limit, layout(cap, mcap, *p2, true).fixed, layout(cap, mcap, *p2, false).fixed, cap, nitems,
                    {kMaxBlocks, kGlobalBlocks, kGlobalRoom}, path);
}

inline void fill_levels(float (&dst)[kMaxLevels], const float* sf, int nlevels) {
  for (int l = 0; l < kMaxLevels; l++) dst[l] = l < nlevels ? sf[l] : 0.0f;
}

}  // namespace win
}  // namespace side
}  // namespace orbx
