/* orbx_stereo.h — the batched stereo front-end: Frame::ComputeStereoMatches (src/Frame.cc:811-981) for B rectified pinhole pairs at once,
 * on the pyramids two product contexts left resident by their last batch extraction, plus the whole stereo front-end of a batch (both
 * extractions and the association) in one call.  Not part of the drop-in boundary (include/orbx.h): these entry points live in
 * liborbx_stereo.so, which links liborbx.so and reads the buffers a product context left behind (orbx_internal.h), the way liborbx_debug.so
 * does.  Per frame the results are bit-identical to orbx_stereo_matches on the same pair.
 *
 * A handle holds scratch memory, one stream and events of its own; calls on one handle run one after the other (each waits, on the device,
 * for the previous one).  orbx_stereo_match_batch_device changes neither context: orbx_stereo_matches keeps working on them before and after.
 * The two extract forms re-run both contexts' batch extractions, as orbx_extract_batch(_device) would, and leave the contexts exactly as those
 * calls leave them.  A context never holds memory of the handle, so the handle may be destroyed before the contexts.
 * ORBX_STEREO_TILE (1 .. 2048: right gates per LDS tile) and ORBX_STEREO_FILTER_LDS (0 .. 12288: the median filter's SADs kept in LDS, larger
 * frames read global memory) in the environment at orbx_stereo_create select smaller values of the two limits; results do not change. */
#ifndef ORBX_STEREO_H
#define ORBX_STEREO_H

#include <stddef.h>
#include <stdint.h>

#include "orbx.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#define ORBX_STEREO_EXPORT __attribute__((visibility("default")))
#else
#define ORBX_STEREO_EXPORT
#endif

typedef struct orbx_stereo orbx_stereo;

/* A rectified rig: two distinct product contexts on ONE device with identical extractor parameters (nfeatures, levels, scale factor, FAST
 * thresholds and the five result-changing options of the CPU profile), as in Frame's stereo constructor (src/Frame.cc:122-141).
 * mb = baseline, mbf = baseline * fx (include/Frame.h).  ORBX_E_INVALID for a mismatch or mb <= 0 (reason: orbx_stereo_last_error(NULL)). */
ORBX_STEREO_EXPORT int orbx_stereo_create(orbx_stereo** out, orbx_ctx* left, orbx_ctx* right, float mb, float mbf);
ORBX_STEREO_EXPORT void orbx_stereo_destroy(orbx_stereo* s);
/* The reason of the handle's last failure; with s = NULL the calling thread's last orbx_stereo_create failure. */
ORBX_STEREO_EXPORT const char* orbx_stereo_last_error(const orbx_stereo* s);

/* ComputeStereoMatches for frames [0, nframes) of the LAST batch extraction of each context, lapping area (0, 0).  Asynchronous on `stream`,
 * which the caller has ordered after both extractions; the caller's input frames (level 0, read in place) stay alive until it has run.
 * d_kps* / d_desc* / d_counts*: [nframes][capacity] / [nframes][capacity][32] / [nframes][2] as orbx_extract_batch_device wrote them;
 * capacity = orbx_keypoint_capacity(left).
 * d_u_right / d_depth: [nframes][capacity] float = mvuRight / mvDepth, -1 where no match and in every slot past the frame's left count;
 * d_kept: [nframes] int32 = matches kept after the median filter, 0 for a frame with no left or no right keypoint, -1 for a frame whose
 * left or right count is -1 (its u_right / depth are all -1).  A NULL stream is the left context's own stream (the one
 * orbx_extract_batch_device takes for a NULL stream).
 * ORBX_E_INVALID when nframes < 1 or exceeds either context's last batch, when the two last batches differ in shape, or when the contexts'
 * parameters no longer agree. */
ORBX_STEREO_EXPORT int orbx_stereo_match_batch_device(orbx_stereo* s, int nframes, const orbx_keypoint* d_kpsL, const uint8_t* d_descL,
                                                      const int32_t* d_countsL, const orbx_keypoint* d_kpsR, const uint8_t* d_descR,
                                                      const int32_t* d_countsR, float* d_u_right, float* d_depth, int32_t* d_kept, void* stream);

/* The whole stereo front-end of a batch in one call: orbx_extract_batch_device of the left frames on `stream` and of the right frames on the
 * right context's own stream (forked from and joined back into `stream` by events), lapping (0, 0), then the call above.  Both sides share the
 * frame layout (row r of frame f at d_imgs + f*frame_stride + r*row_stride).  Asynchronous on `stream`. */
ORBX_STEREO_EXPORT int orbx_stereo_extract_batch_device(orbx_stereo* s, const uint8_t* d_imgsL, const uint8_t* d_imgsR, int nframes, int rows,
                                                        int cols, size_t row_stride, size_t frame_stride, orbx_keypoint* d_kpsL,
                                                        uint8_t* d_descL, int32_t* d_countsL, orbx_keypoint* d_kpsR, uint8_t* d_descR,
                                                        int32_t* d_countsR, float* d_u_right, float* d_depth, int32_t* d_kept, void* stream);

/* Host-buffer convenience: orbx_extract_batch on each side (the frames are staged in memory the context owns, so level 0 of the batch stays
 * valid after the handle is gone), then the association on the uploaded results and the read-back; returns when the results are in the
 * caller's buffers.  Output layouts as above, in host memory. */
ORBX_STEREO_EXPORT int orbx_stereo_extract_batch(orbx_stereo* s, const uint8_t* imgsL, const uint8_t* imgsR, int nframes, int rows, int cols,
                                                 size_t row_stride, size_t frame_stride, orbx_keypoint* kpsL, uint8_t* descL, int32_t* countsL,
                                                 orbx_keypoint* kpsR, uint8_t* descR, int32_t* countsR, float* u_right, float* depth,
                                                 int32_t* kept);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_STEREO_H */
