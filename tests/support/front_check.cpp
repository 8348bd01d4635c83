// The plain-C++ part of csrc/side/orbx_front_device.h and orbx_front_host.h on the host (tests/test_front_core.py): the counting level the
// kernels run against the libm level of the host twins, and the shared argument checks.
//   levels  for log_scale_factor in {logf(1.2f), logf(2.0f)}, nlevels in {1, 2, 8, 16} and both log kinds the thresholds are bisected
//           (level_thresholds) and put into the kernel arguments' tables (fill_levels); count_level, with and without the scale factor, must
//           equal HostLevel on the 4096 floats on either side of every threshold and at 0, -0.0f, a subnormal, FLT_MAX, +inf, -1 and a NaN,
//           and the picked scale factor must be sf[level].  The tables must hold +inf past nlevels - 2 and the last factor past nlevels - 1.
//   checks  every reason of thresholds_problem, log_problem, common_problem and grid_problem on planted arguments, in their order.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

#include "../../orb_slam3_modified_amd/csrc/side/orbx_front_host.h"

using namespace orbx::side::front;

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static long g_bad = 0, g_done = 0;
static void same(bool ok, const char* what, double a = 0, double b = 0) {
  g_done++;
  if (!ok && g_bad++ < 20) printf("MISMATCH %s (%a, %a)\n", what, a, b);
}
static void reason(const char* got, const char* want, const char* what) {
  g_done++;
  const bool ok = want ? got && !strcmp(got, want) : !got;
  if (!ok && g_bad++ < 20) printf("MISMATCH %s: got '%s', want '%s'\n", what, got ? got : "(none)", want ? want : "(none)");
}

static void one_ratio(const HostLevel& host, const float* T, const float* sf, float ratio) {
  int want;
  float want_scale, scale = -1.0f, unused = -1.0f;
  host(ratio, &want, &want_scale);
  const int got = count_level<true>(T, sf, ratio, &scale);
  same(got == want && host(ratio) == want, "level", ratio, got);
  same(bits(scale) == bits(sf[want]) && bits(scale) == bits(want_scale), "scale", ratio, scale);
  same(count_level<false>(T, nullptr, ratio, &unused) == want && unused == 0.0f, "level without scale", ratio);
}

static void levels(float lsf, int nlevels, int log_kind) {
  float raw[kMaxT], factors[kMaxLevels], T[kMaxT], sf[kMaxLevels];
  std::string why;
  const char* e = level_thresholds(lsf, nlevels, log_kind, raw, &why);
  same(e == nullptr, e ? e : "level_thresholds", lsf, nlevels);
  if (e) return;
  for (int n = 0; n < nlevels; n++) factors[n] = n ? factors[n - 1] * 1.2f : 1.0f;
  fill_levels(T, sf, nlevels > 1 ? raw : nullptr, factors, nlevels);
  reason(thresholds_problem(nlevels > 1 ? raw : nullptr, nlevels), nullptr, "bisected thresholds");
  for (int n = 0; n < kMaxT; n++) same(n + 1 < nlevels ? bits(T[n]) == bits(raw[n]) : T[n] == INFINITY, "T", n, T[n]);
  for (int n = 0; n < kMaxLevels; n++) same(bits(sf[n]) == bits(factors[n < nlevels ? n : nlevels - 1]), "sf", n, sf[n]);
  const HostLevel host = {lsf, nlevels, log_kind, factors};
  for (int n = 0; n + 1 < nlevels; n++) {
    const uint32_t at = bits(T[n]);
    for (uint32_t k = 0; k < 4096; k++) {
      if (at >= 1u + k) one_ratio(host, T, sf, from_bits(at - k));
      if (at + 1u + k <= 0x7F7FFFFFu) one_ratio(host, T, sf, from_bits(at + 1u + k));
    }
  }
  for (float r : {0.0f, -0.0f, from_bits(1u), from_bits(0x007FFFFFu), FLT_MAX, INFINITY, -1.0f, std::numeric_limits<float>::quiet_NaN()})
    one_ratio(host, T, sf, r);
  // without thresholds or scale factors: level 0 everywhere, zeros
  fill_levels(T, sf, nullptr, nullptr, nlevels);
  for (int n = 0; n < kMaxT; n++) same(T[n] == INFINITY, "T without thresholds", n);
  for (int n = 0; n < kMaxLevels; n++) same(bits(sf[n]) == 0u, "sf without factors", n);
}

static void checks() {
  const char* kLevels = "nlevels must be in 1 .. 16";
  const char* kFinite = "thresholds must be finite and positive";
  const char* kOrder = "thresholds must be strictly increasing";
  const float good[3] = {1.0f, 1.5f, 2.0f};
  reason(thresholds_problem(good, 4), nullptr, "good thresholds");
  reason(thresholds_problem(good, 0), kLevels, "nlevels 0");
  reason(thresholds_problem(good, 17), kLevels, "nlevels 17");
  reason(thresholds_problem(nullptr, 2), "null thresholds", "null thresholds");
  reason(thresholds_problem(nullptr, 1), nullptr, "one level needs no thresholds");
  for (float v : {std::numeric_limits<float>::quiet_NaN(), INFINITY, 0.0f, -0.0f, -1.0f})
    for (int at = 0; at < 3; at++) {
      float T[3] = {1.0f, 1.5f, 2.0f};
      T[at] = v;
      reason(thresholds_problem(T, 4), kFinite, "a threshold that is not finite and positive");
    }
  const float equal[3] = {1.0f, 1.5f, 1.5f}, down[3] = {1.0f, 2.0f, 1.5f};
  reason(thresholds_problem(equal, 4), kOrder, "equal thresholds");
  reason(thresholds_problem(down, 4), kOrder, "descending thresholds");
  reason(thresholds_problem(down, 2), nullptr, "thresholds past nlevels - 2 are not read");

  const float lsf = logf(1.2f);
  reason(log_problem(lsf, 8, ORBX_FRUSTUM_LOG_FLOAT), nullptr, "good log");
  reason(log_problem(lsf, 0, 0), kLevels, "log: nlevels 0");
  reason(log_problem(lsf, 17, 5), kLevels, "log: nlevels before log_kind");
  reason(log_problem(-1.0f, 8, 2), "unknown log_kind", "log_kind before log_scale_factor");
  for (float v : {std::numeric_limits<float>::quiet_NaN(), INFINITY, 0.0f, -0.1f})
    reason(log_problem(v, 8, 0), "log_scale_factor must be finite and positive", "log_scale_factor");
  reason(rot_problem(ORBX_PROJECT_ROT_QUAT), nullptr, "rot_kind");
  reason(rot_problem(2), "unknown rot_kind", "rot_kind 2");
  reason(sum_problem(ORBX_FRUSTUM_SUM_TREE), nullptr, "sum_order");
  reason(sum_problem(-1), "unknown sum_order", "sum_order -1");

  const char* kSizes = "npoints, nitems and mcap must be at least 1";
  reason(common_problem(nullptr, 1, 1, 1, nullptr), nullptr, "good call");
  reason(common_problem("null x", 0, 1, 1, "own"), "null x", "nulls first");
  reason(common_problem(nullptr, 0, 1, 1, "own"), kSizes, "npoints 0");
  reason(common_problem(nullptr, 1, 0, 1, "own"), kSizes, "nitems 0");
  reason(common_problem(nullptr, 1, 1, 0, "own"), kSizes, "mcap 0");
  reason(common_problem(nullptr, 1, 1 << 20, 1 << 12, "own"), "own", "the library's own before the product");
  reason(common_problem(nullptr, 1, 1 << 20, 1 << 12, nullptr), "nitems * mcap exceeds INT_MAX", "the product");
  reason(common_problem(nullptr, 1, 1 << 20, (1 << 11) - 1, nullptr), nullptr, "below INT_MAX");

  int chunks = -1;
  reason(grid_problem(0x1008, "unaligned", 1, 1, &chunks), "unaligned", "alignment");
  reason(grid_problem(0x1010, "unaligned", 3, 257, &chunks), nullptr, "grid");
  same(chunks == 2, "chunks of 257 slots", chunks);
  reason(grid_problem(0, nullptr, 3, 256, &chunks), nullptr, "grid");
  same(chunks == 1, "chunks of 256 slots", chunks);
  reason(grid_problem(0, nullptr, 1 << 24, 1 << 16, &chunks), "too many workgroups", "2^24 items of 2^8 chunks");
}

int main() {
  for (float lsf : {logf(1.2f), logf(2.0f)})
    for (int nlevels : {1, 2, 8, 16})
      for (int log_kind : {ORBX_FRUSTUM_LOG_DOUBLE, ORBX_FRUSTUM_LOG_FLOAT}) levels(lsf, nlevels, log_kind);
  printf("levels: %ld comparisons, %ld mismatches\n", g_done, g_bad);
  const long before = g_done, bad_before = g_bad;
  checks();
  printf("checks: %ld comparisons, %ld mismatches\n", g_done - before, g_bad - bad_before);
  return 0;
}
