/* orbx_initmatch.h — the batched SearchForInitialization: ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:648-763) for P (frame, frame)
 * pairs at once, on the keypoints, descriptors and counts a batch extraction left in HBM.  No vocabulary, no map points, no poses.  Not part
 * of the drop-in boundary (include/orbx.h): these entry points live in liborbx_initmatch.so.  The library reads plain device arrays only.
 *
 * The specification is the reference's loop.  For pair p = (ia, ib), F1 = frame ia of side a (the queries), F2 = frame ib of side b:
 *   grid   F2's keypoints are put into the 64 x 48 frame grid (src/Frame.cc:385-416, :725-735), in float arithmetic that is not contracted:
 *            invW = 64.0f / (maxX - minX), invH = 48.0f / (maxY - minY),
 *            posX = (int)round((x - minX) * invW), posY = (int)round((y - minY) * invH)   (std::round: halves away from zero);
 *          a keypoint whose cell lies outside the grid is in no cell.  Inside a cell the keypoints stand in ascending index.
 *   query  the F1 keypoints with octave == 0, in ascending index i1; every other F1 keypoint keeps -1.  (The extractor's octaves are
 *          0 .. nlevels - 1.  A negative octave counts as "not level 0" on both sides.)
 *   window GetFeaturesInArea(c.x, c.y, r = (float)window_size, 0, 0) (src/Frame.cc:657-723), c = prev_xy[i1]:
 *            nMinCellX = max(0, (int)floor((c.x - minX - r) * invW)), no candidate when >= 64;
 *            nMaxCellX = min(63, (int)ceil((c.x - minX + r) * invW)), no candidate when < 0; the same in y with invH and 48 (the four early
 *            returns, in this order);
 *          the cells are walked x-major, then y, then the cell's keypoints in ascending index; a keypoint is a candidate when its
 *          octave == 0 and fabs(x - c.x) < r && fabs(y - c.y) < r (strict).  This order decides ties.
 *   scan   over the candidates i2 in that order, dist = the Hamming distance of the two descriptors: a candidate with
 *          vMatchedDistance[i2] <= dist is skipped (an F2 feature held at distance d is taken only by a strictly closer query); bestDist is
 *          the first minimum in list order (strict <), bestDist2 the second smallest of the multiset, ties included; BOTH START AT INT_MAX.
 *   accept when bestDist <= 50 and (float)bestDist < (float)bestDist2 * nn_ratio (one float multiplication, not contracted; with one
 *          surviving candidate the right side is (float)INT_MAX * nn_ratio).  Then: the query that held bestIdx2 before, if any, loses its
 *          match (-1); vnMatches12[i1] = bestIdx2; vMatchedDistance[bestIdx2] = bestDist; with check_orientation the acceptance is entered
 *          into the rotation histogram: rot = angle1[i1] - angle2[bestIdx2], + 360.0f when negative, bin = (int)round(rot * (1.0f / 30)),
 *          bin 30 -> 0.  The entry stays when the match is stolen later: push_back is never undone.
 *   filter with check_orientation, after the last query: ComputeThreeMaxima (src/ORBmatcher.cc:2012-2053) over the 30 bin sizes; every query
 *          whose recorded bin is none of the three and whose match is still >= 0 loses it.
 *   prev   prev_xy[i1] = F2's keypoint position for every i1 with vnMatches12[i1] >= 0; the return value is the number of those i1.
 *
 * What is parallel and what is not: the grid, every window's candidate list and every candidate's Hamming distance depend on the inputs alone
 * and are computed by a whole workgroup per pair.  vMatchedDistance makes the scan of query i1 depend on every earlier acceptance anywhere in
 * the frame: that chain runs on one wave per pair over the precomputed distances (no descriptor is touched in it), P chains at once.  The
 * histogram needs each acceptance's bin and the bin SIZES only, so it is counted after the chain, in parallel, from the F2 feature every query
 * held when it was accepted.  Results do not depend on scheduling or on the path (LDS or global memory).
 *
 * A handle holds scratch memory, one stream and one event of its own; calls on one handle run one after the other on the device.
 * Environment, read at orbx_initmatch_create (results do not change): ORBX_INITMATCH_LDS = the largest LDS block in bytes a call may keep a
 * pair in (0 .. 155648; capacities that need more run on global memory). */
#ifndef ORBX_INITMATCH_H
#define ORBX_INITMATCH_H

#include <stddef.h>
#include <stdint.h>

#include "orbx.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#define ORBX_INITMATCH_EXPORT __attribute__((visibility("default")))
#else
#define ORBX_INITMATCH_EXPORT
#endif

typedef struct orbx_initmatch orbx_initmatch;

/* One side of the pairs: a batch of frames at fixed stride, as orbx_extract_batch_device leaves it. */
typedef struct orbx_initmatch_side {
  const orbx_keypoint* d_kps;   /* [nframes][capacity]: the frame's mvKeysUn; x, y, angle, octave are read */
  const uint8_t* d_desc;        /* [nframes][capacity][32] */
  const int32_t* d_counts;      /* [nframes][2]: {keypoints, -} */
  int nframes, capacity;
} orbx_initmatch_side;

/* ORBX_E_INVALID for out = NULL or device < 0, ORBX_E_DEVICE when the device cannot be opened (reason: orbx_initmatch_last_error(NULL)). */
ORBX_INITMATCH_EXPORT int orbx_initmatch_create(orbx_initmatch** out, int device);
ORBX_INITMATCH_EXPORT void orbx_initmatch_destroy(orbx_initmatch* m);
/* The reason of the handle's last failure; with m = NULL the calling thread's last orbx_initmatch_create failure. */
ORBX_INITMATCH_EXPORT const char* orbx_initmatch_last_error(const orbx_initmatch* m);

/* SearchForInitialization for pairs [0, npairs): d_pairs [npairs][2] int32 = {frame of a, frame of b}; a and b may be the same batch.
 *   bounds      {mnMinX, mnMinY, mnMaxX, mnMaxY} of side b's frames (host memory)
 *   d_prev_xy   [npairs][a.capacity][2] float, in/out: vbPrevMatched, one row per pair.  Read as the window centres; on return row i1 holds
 *               F2's matched point wherever d_matches12[i1] >= 0, every other row is untouched.  NULL: the centres are F1's own keypoint
 *               positions (src/Tracking.cc:2470-2472) and nothing is written back.
 *   d_matches12 [npairs][a.capacity] int32   vnMatches12: the F2 feature of F1 feature i1, -1 for none
 *   d_matches21 [npairs][b.capacity] int32   the exact inverse of the final d_matches12 (not the reference's internal vnMatches21, which keeps
 *               stale entries), or NULL
 *   d_nmatches  [npairs] int32               the reference's return value
 * Whole rows are written (-1 past the frame's count).  A pair is malformed when a frame index lies outside its batch or a count is negative
 * or above `capacity`: then d_nmatches[p] = -1, its rows are all -1 and its prev_xy rows are untouched.  This is checked on the device, and
 * every index that addresses memory is clamped first.  Asynchronous on `stream`; NULL is the handle's own stream.
 * ORBX_E_INVALID for what the host can check: NULL arguments, sizes < 1, window_size < 0, bounds with max <= min, a capacity above 32768 (the
 * device-built grid's index width), npairs * capacity beyond INT_MAX, buffers on another device than the handle's. */
ORBX_INITMATCH_EXPORT int orbx_initmatch_pairs_device(orbx_initmatch* m, const orbx_initmatch_side* a, const orbx_initmatch_side* b,
                                                      const int32_t* d_pairs, int npairs, const float bounds[4], int window_size, float nn_ratio,
                                                      int check_orientation, float* d_prev_xy, int32_t* d_matches12, int32_t* d_matches21,
                                                      int32_t* d_nmatches, void* stream);

/* The same call on host arrays of the same fixed-stride layout (the d_ members of a and b, pairs, prev_xy and the results are host pointers
 * here); returns when the results are in the caller's buffers. */
ORBX_INITMATCH_EXPORT int orbx_initmatch_pairs(orbx_initmatch* m, const orbx_initmatch_side* a, const orbx_initmatch_side* b,
                                               const int32_t* pairs, int npairs, const float bounds[4], int window_size, float nn_ratio,
                                               int check_orientation, float* prev_xy, int32_t* matches12, int32_t* matches21, int32_t* nmatches);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_INITMATCH_H */
