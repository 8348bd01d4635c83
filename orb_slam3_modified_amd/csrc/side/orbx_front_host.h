// The host side the three projection fronts share (liborbx_frustum.so, liborbx_project.so, liborbx_sim3.so): the level as libm computes
// it and the thresholds bisected through it, the argument checks, the kernel arguments' level tables, the option dispatch and the host
// twins' loop.  Plain C++, no HIP: tests/support/front_check.cpp compiles it with the host compiler.
#pragma once
#include <climits>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>

#include "orbx_front_device.h"

namespace orbx {
namespace side {
namespace front {

// ---------------------------------------------------------------------------------------------------------------- the level on the host
// ceil(log(ratio) / mfLogScaleFactor) as the C++ expression evaluates under each overload of log, before the conversion to int
inline double level_quotient(float ratio, float lsf, int log_kind) {
  if (log_kind == ORBX_FRUSTUM_LOG_FLOAT) {
    const float q = std::log(ratio) / lsf;          // std::log(float): libm's logf, a float division
    return std::ceil((double)q);
  }
  return std::ceil(::log((double)ratio) / (double)lsf);   // ::log(double), the float divisor promoted
}
// int nScale = <quotient>, then the clamp.  Outside the range of int (NaN included) x86's conversion gives INT_MIN, which the clamp raises
// to 0 (include/orbx_frustum.h, step 9 and Limits)
inline int level_clamp(double q, int nlevels) {
  if (!(q >= -2147483648.0 && q < 2147483648.0)) return 0;
  const int n = (int)q;
  return n < 0 ? 0 : n >= nlevels ? nlevels - 1 : n;
}
struct HostLevel {   // sf: the scale factors, or null; frustum's form returns the level alone
  float lsf; int nlevels, log_kind; const float* sf;
  int operator()(float ratio) const { return level_clamp(level_quotient(ratio, lsf, log_kind), nlevels); }
  void operator()(float ratio, int* lvl, float* scale) const {
    *lvl = (*this)(ratio);
    *scale = sf ? sf[*lvl] : 0.0f;
  }
};
struct HostPoints {
  const orbx_frustum_point* t;
  const orbx_frustum_point& operator()(int idx) const { return t[idx]; }
};

inline float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

// T[n], n in 0 .. nlevels-2: the largest positive finite float whose level is <= n.  Why it cannot be had, or nullptr.  Reached from
// liborbx_frustum.so alone: the other two take the thresholds from their caller.
inline const char* level_thresholds(float lsf, int nlevels, int log_kind, float* T, std::string* why) {
  const HostLevel level = {lsf, nlevels, log_kind, nullptr};
  constexpr uint32_t kLo = 1u, kHi = 0x7F7FFFFFu;   // the smallest subnormal, FLT_MAX
  // the quotient stays within int over all positive floats, so the x86 rule never cuts into the step
  for (uint32_t e : {kLo, kHi}) {
    const double q = level_quotient(from_bits(e), lsf, log_kind);
    if (!(q >= -2147483648.0 && q < 2147483648.0)) return "log_scale_factor is too small: the level quotient leaves the range of int";
  }
  if (level(from_bits(kLo)) != 0) return "the smallest positive ratio does not have level 0";
  for (int n = 0; n + 1 < nlevels; n++) {
    uint32_t lo = kLo, hi = kHi;                   // level(lo) <= n throughout
    if (level(from_bits(hi)) <= n) lo = hi;        // no finite ratio reaches level n + 1
    while (hi - lo > 1 && lo != hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (level(from_bits(mid)) <= n) lo = mid; else hi = mid;
    }
    T[n] = from_bits(lo);
    // the step itself: 4096 floats on either side
    for (uint32_t k = 0; k < 4096; k++) {
      const bool below_ok = lo < kLo + k || level(from_bits(lo - k)) <= n;
      const bool above_ok = lo + 1 + k > kHi || level(from_bits(lo + 1 + k)) > n;
      if (!below_ok || !above_ok) {
        char buf[160];
        snprintf(buf, sizeof buf, "the level is not a clean step of ratio around %a (level %d, log_scale_factor %a, log_kind %d)", (double)T[n], n,
                 (double)lsf, log_kind);
        *why = buf;
        return why->c_str();
      }
    }
    if (n > 0 && T[n] < T[n - 1]) return "the thresholds do not ascend";
  }
  return nullptr;
}

// ------------------------------------------------------------------------------------------------------- the checks; a reason, or nullptr
inline const char* rot_problem(int rot_kind) {
  return rot_kind != ORBX_PROJECT_ROT_MATRIX && rot_kind != ORBX_PROJECT_ROT_QUAT ? "unknown rot_kind" : nullptr;
}
inline const char* sum_problem(int sum_order) {
  return sum_order != ORBX_FRUSTUM_SUM_LTR && sum_order != ORBX_FRUSTUM_SUM_TREE ? "unknown sum_order" : nullptr;
}
inline bool usable_lsf(float lsf) { return std::isfinite(lsf) && lsf > 0.0f; }
inline const char* levels_problem(int nlevels) { return nlevels < 1 || nlevels > kMaxLevels ? "nlevels must be in 1 .. 16" : nullptr; }
inline const char* thresholds_problem(const float* T, int nlevels) {
  if (const char* e = levels_problem(nlevels)) return e;
  if (!T && nlevels > 1) return "null thresholds";
  for (int n = 0; n + 1 < nlevels; n++) {
    if (!std::isfinite(T[n]) || !(T[n] > 0.0f)) return "thresholds must be finite and positive";
    if (n > 0 && !(T[n] > T[n - 1])) return "thresholds must be strictly increasing";
  }
  return nullptr;
}
inline const char* log_problem(float lsf, int nlevels, int log_kind) {
  if (const char* e = levels_problem(nlevels)) return e;
  if (log_kind != ORBX_FRUSTUM_LOG_DOUBLE && log_kind != ORBX_FRUSTUM_LOG_FLOAT) return "unknown log_kind";
  if (!usable_lsf(lsf)) return "log_scale_factor must be finite and positive";
  return nullptr;
}
// what every library's call_problem has in common.  `missing`: the library's words for a null pointer among its arguments, `own`: the
// problem of its own options; either may be nullptr
inline const char* common_problem(const char* missing, int npoints, int nitems, int mcap, const char* own) {
  if (missing) return missing;
  if (npoints < 1 || nitems < 1 || mcap < 1) return "npoints, nitems and mcap must be at least 1";
  if (own) return own;
  if ((long long)nitems * mcap > (long long)INT_MAX) return "nitems * mcap exceeds INT_MAX";
  return nullptr;
}
// what a device form checks first: `pointers` (or-ed together) against 16 bytes, with the library's words for it; the chunks of 256 slots
// of one item; the grid of nitems * chunks workgroups
inline const char* grid_problem(uintptr_t pointers, const char* unaligned, int nitems, int mcap, int* chunks) {
  if (pointers & 15) return unaligned;
  *chunks = (mcap + kThreads - 1) / kThreads;
  if ((long long)nitems * *chunks > (long long)INT_MAX) return "too many workgroups";
  return nullptr;
}

// the kernel arguments' tables: T +inf past nlevels - 2 (or without thresholds), sf (where the library has one) the last factor repeated
// past nlevels - 1 (zeros without scale factors)
inline void fill_levels(float (&T)[kMaxT], float* sf, const float* thresholds, const float* scale_factors, int nlevels) {
  for (int n = 0; n < kMaxT; n++) T[n] = (thresholds && n + 1 < nlevels) ? thresholds[n] : INFINITY;
  for (int n = 0; sf && n < kMaxLevels; n++) sf[n] = scale_factors ? scale_factors[n < nlevels ? n : nlevels - 1] : 0.0f;
}

// ------------------------------------------------------------------------------------------------------------ the options, the host twin
// f(c) with c a std::true_type or std::false_type: `v` as a compile-time constant, c() in a template argument
template <class F>
inline auto pick(bool v, F f) { return v ? f(std::true_type{}) : f(std::false_type{}); }
// f(quat, tree): rot_kind and sum_order as compile-time constants
template <class F>
inline auto dispatch(int rot_kind, int sum_order, F f) {
  return pick(rot_kind == ORBX_PROJECT_ROT_QUAT, [&](auto q) { return pick(sum_order == ORBX_FRUSTUM_SUM_TREE, [&](auto t) { return f(q, t); }); });
}

// The host twin's loop: per item the check, then emit(b, s, &r) for each of its first nslots[b] slots (s: the slot's `stride` words, the
// point's index the first), `skipped` for the others; out [nitems, mcap] rows, nvalid[b] the valid rows or -1.
template <class E>
inline void reference(const int32_t* slots, int stride, const int32_t* nslots, int nitems, int mcap, int npoints, const Row& skipped, void* out,
                      int32_t* nvalid, E emit) {
  for (int b = 0; b < nitems; b++) {
    const int32_t* row = slots + (size_t)b * mcap * stride;
    bool bad = nslots[b] < 0 || nslots[b] > mcap;
    for (int j = 0; !bad && j < nslots[b]; j++) bad = row[(size_t)j * stride] >= npoints;
    const int n = bad ? 0 : nslots[b];
    int count = 0;
    for (int j = 0; j < mcap; j++) {
      Row r = skipped;
      if (j < n) count += emit(b, row + (size_t)j * stride, &r);
      memcpy((uint8_t*)out + ((size_t)b * mcap + j) * sizeof(Row), &r, sizeof(Row));
    }
    nvalid[b] = bad ? -1 : count;
  }
}

}  // namespace front
}  // namespace side
}  // namespace orbx
