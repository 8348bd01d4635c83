// What makes the two extractions of a two-camera pair comparable (liborbx_stereo.so, liborbx_fisheye.so): Frame's stereo constructors build
// both extractors from one set of settings.  Host code only; it sits below csrc/, outside kernels_hash().
#pragma once
#include "../orbx_internal.h"

namespace orbx {
namespace side {

// why the two contexts are no rig, or nullptr
inline const char* rig_mismatch(const orbx_ctx* a, const orbx_ctx* b) {
  if (a->device != b->device) return "the two contexts live on different devices";
  if (a->nfeatures != b->nfeatures || a->nlevels != b->nlevels || a->scale_factor != b->scale_factor || a->ini_th != b->ini_th ||
      a->min_th != b->min_th)
    return "the two contexts have different extractor parameters (nfeatures, levels, scale factor, FAST thresholds)";
  if (a->gauss_kernel != b->gauss_kernel || a->gauss_round != b->gauss_round || a->gauss_tail != b->gauss_tail || a->atan_fma != b->atan_fma ||
      a->brief_fma != b->brief_fma)
    return "the two contexts have different CPU profiles (gauss_kernel, gauss_round, gauss_tail, atan_fma, brief_fma)";
  return nullptr;
}

}  // namespace side
}  // namespace orbx
