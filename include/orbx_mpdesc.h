/* orbx_mpdesc.h — the batched MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:329-403) for M map points at once, on the
 * descriptors a batch extraction left in HBM: of a point's N observed descriptors the one whose median Hamming distance to the others is
 * least.  The reference calls it for every map point CreateNewMapPoints, SearchInNeighbors, loop fusion and the tracking thread touched
 * (src/LocalMapping.cc:323,704,815, src/LoopClosing.cc:1130, src/MapPoint.cc:297, src/Tracking.cc:2393,2414,2562,3316).  Not part of the
 * drop-in boundary (include/orbx.h): these entry points live in liborbx_mpdesc.so.  The library reads plain device arrays only; it takes
 * nothing from a context.  The winners are written as rows of a descriptor table, which is what orbx_fuse_search_device (orbx_fuse.h) reads
 * as d_pdesc: between extraction, triangulation, fuse and the next fuse the descriptors stay in HBM.
 *
 * In scope: what is a pure function of the observed descriptors -- the N x N distances, each row's median, the least median, the copy.
 * Out of scope:
 *   the observation list itself (mObservations, isBad(), the mutexes): host pointer work.  The caller lists a point's observations in the
 *     order the reference's loop pushes them (:348-363): its std::map iteration order, the left row before the right row, bad keyframes
 *     left out.  On a two-camera rig the right observation is simply another row of the same keyframe's stacked mDescriptors;
 *   mbBad: the caller leaves a bad point out, or lists it with no observation.
 *
 * The specification is the reference's loop.  For point m the observations are d_obs[d_obs_start[m] .. d_obs_start[m + 1]), N of them;
 * observation i names row `row` of keyframe `frame` of the side.  The same (frame, row) may appear in many points and twice in one.
 *   D[i][j]   the Hamming distance of the descriptors of observations i and j (:372-381); D[i][i] = 0.
 *   median_i  the element at index (int)(0.5 * (N - 1)) of row i sorted ascending (:388-390): the lower middle for an even N, and for
 *             N <= 2 the self-distance 0.
 *   winner    the smallest median_i; the first i wins a tie (strict < from INT_MAX, :384-397).
 *   result    d_best[m] = the winner's index in the point's list, d_median[m] = its median, and its 32 bytes are copied to row
 *             d_out_row[m] of d_out_desc (row m when d_out_row is NULL).  The caller keeps the out rows of one call distinct.
 *   N == 0    the reference returns early (:365): d_best[m] = -1, d_median[m] = -1, the output row is not touched.
 * A malformed point gets d_best[m] = -2, d_median[m] = -1 and an untouched output row; every other point of the call is unaffected.  A
 * point is malformed when d_obs_start[m] < 0, d_obs_start[m + 1] < d_obs_start[m] or d_obs_start[m + 1] > nobs; when N exceeds
 * ORBX_MPDESC_MAX_OBS; when its out row lies outside 0 .. out_rows - 1; when an observation's frame lies outside 0 .. nframes - 1 or its
 * row outside 0 .. min(d_counts[frame][0], capacity) - 1.  All of it is checked on the device before any of these values addresses memory.
 * Nothing is ordered; the result does not depend on scheduling.
 *
 * Limit: at most ORBX_MPDESC_MAX_OBS = 1024 observations a point.  It is a limit of this library, stated as one; the reference's
 * `float Distances[N][N]` on the stack ends near N = 1400 of itself (8 MiB).
 *
 * A handle holds scratch memory, one stream and one event of its own; calls on one handle run one after the other on the device.
 * Environment, read at orbx_mpdesc_create (results do not change): ORBX_MPDESC_SMALL_MAX = the largest N of the lane-per-observation form
 * (0 .. 64), ORBX_MPDESC_MID_MAX = the largest N of the workgroup-per-point form that keeps the distances in LDS (0 .. 256); points
 * above both take the form that recomputes them. */
#ifndef ORBX_MPDESC_H
#define ORBX_MPDESC_H

#include <stddef.h>
#include <stdint.h>

#include "orbx.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#define ORBX_MPDESC_EXPORT __attribute__((visibility("default")))
#else
#define ORBX_MPDESC_EXPORT
#endif

#define ORBX_MPDESC_MAX_OBS 1024

typedef struct orbx_mpdesc orbx_mpdesc;

/* The descriptor side: K keyframes at fixed stride, the buffers a batch extraction leaves (orbx_fuse_side without keypoints and grids). */
typedef struct orbx_mpdesc_side {
  const uint8_t* d_desc;        /* [nframes][capacity][32], 16-byte aligned */
  const int32_t* d_counts;      /* [nframes][2]: {descriptor rows, -} */
  int nframes, capacity;
} orbx_mpdesc_side;

/* One observation: row `row` of keyframe `frame`. */
typedef struct orbx_mpdesc_obs {
  int32_t frame, row;
} orbx_mpdesc_obs;

/* ORBX_E_INVALID for out = NULL or device < 0, ORBX_E_DEVICE when the device cannot be opened (reason: orbx_mpdesc_last_error(NULL)). */
ORBX_MPDESC_EXPORT int orbx_mpdesc_create(orbx_mpdesc** out, int device);
ORBX_MPDESC_EXPORT void orbx_mpdesc_destroy(orbx_mpdesc* m);
/* The reason of the handle's last failure; with m = NULL the calling thread's last orbx_mpdesc_create failure. */
ORBX_MPDESC_EXPORT const char* orbx_mpdesc_last_error(const orbx_mpdesc* m);

/* The selection for points [0, npoints):
 *   d_obs        [nobs] orbx_mpdesc_obs, d_obs_start [npoints + 1] int32: the observations in CSR form
 *   d_out_row    [npoints] int32, or NULL: point m's row is m
 *   d_out_desc   [out_rows][32], 16-byte aligned: the winners' rows are written, every other row is left as it is
 *   d_best, d_median [npoints] int32
 * Asynchronous on `stream`; NULL is the handle's own stream.  A fixed number of launches whatever the points are, no host
 * synchronisation.
 * ORBX_E_INVALID for what the host can check: NULL arguments, nframes, capacity, nobs, npoints or out_rows < 1, nframes * capacity beyond
 * INT_MAX, a table that is not 16-byte aligned, buffers on another device than the handle's. */
ORBX_MPDESC_EXPORT int orbx_mpdesc_select_device(orbx_mpdesc* m, const orbx_mpdesc_side* side, const orbx_mpdesc_obs* d_obs, int nobs,
                                                 const int32_t* d_obs_start, int npoints, const int32_t* d_out_row, uint8_t* d_out_desc,
                                                 int out_rows, int32_t* d_best, int32_t* d_median, void* stream);

/* The same on host arrays of the same layout (the d_ members of side, the observations, the table and the results are host pointers
 * here): uploads them -- the table too, so that the rows no point writes come back as they were --, selects, and returns when the
 * results are in the caller's buffers. */
ORBX_MPDESC_EXPORT int orbx_mpdesc_select(orbx_mpdesc* m, const orbx_mpdesc_side* side, const orbx_mpdesc_obs* obs, int nobs,
                                          const int32_t* obs_start, int npoints, const int32_t* out_row, uint8_t* out_desc, int out_rows,
                                          int32_t* best, int32_t* median);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_MPDESC_H */
