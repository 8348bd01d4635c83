#!/usr/bin/env python3
"""Batched Fuse search times (liborbx_fuse.so) -> profiles/fuse_times_r12.txt.

256 synthetic frames at the EuRoC shape (752 x 480; 1000 features, 1.2, 8 levels, 20 / 7) resident in HBM as keyframes, monocular, the
reprojection gate on.  The workload has the shape of LocalMapping::SearchInNeighbors with 20 neighbours (the ten frames before and the ten
after, indices modulo 256); a keyframe's "map points" are its own keypoints (position as extracted: the synthetic camera moves 1.5 px right
and 0.5 px down per frame, so the windows of the far neighbours are mostly empty), r = 3 * scale_factor[octave], levels octave - 1 .. octave,
the point's descriptor the keypoint's own (the pool is the batch's descriptor buffer):
  own_into_neighbours   5120 pairs: each keyframe's ~1000 points into each of its 20 neighbours (qcap = capacity)
  neighbours_into_own   256 pairs: each keyframe receives its 20 neighbours' points as one row of ~20 000 queries
Per list:
  (g) orbx_fuse_grids_device for the 256 keyframes, HIP events, `--repeats` runs after three warm-up runs: median [min, max]
  (s) orbx_fuse_search_device, the same way
  (a) the per-pair path the project had before: orbx_target_nearest on a resident target per keyframe, one call per pair with host
      arrays, wall clock per call over a sample of the same pairs; its rows are compared with (s)'s
  (d) the batch extraction and the FeatureVector transform that feed the mapping thread, HIP events
The conditions to check: (s) per pair below (a) per pair, and one keyframe's whole SearchInNeighbors batch -- 1/256 of (g) + both (s) --
below one keyframe's share of (d).
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from times_util import Extracted, stats, timed, write_result  # noqa: E402
OUT = os.path.join(ROOT, "profiles", "fuse_times_r12.txt")
NEIGHBOURS = [j for j in range(-10, 11) if j]


def frame_queries(x, f, scale):
    """Frame f's keypoints as one run of query records, the point being the keypoint's row in the batch's descriptor buffer."""
    from orb_slam3_modified_amd.fuse import QUERY_DTYPE
    n = int(x.hc[f, 0])
    k = x.hk[f, :n]
    q = np.zeros(n, QUERY_DTYPE)
    q["x"], q["y"], q["r"], q["ur"] = k["x"], k["y"], np.float32(3.0) * scale[k["octave"]], -1.0
    q["min_level"], q["max_level"], q["point"] = np.maximum(k["octave"] - 1, 0), k["octave"], f * x.cap + np.arange(n)
    return q


def run(B, repeats, train_frames, sample):
    import torch
    from orb_slam3_modified_amd import ORBextractor, ORBVocabulary, synth
    from orb_slam3_modified_amd.bow import BowBatch
    from orb_slam3_modified_amd.fuse import LDS_MAX, QUERY_DTYPE, FuseBatch, FuseSide, grid_parameters, lds_bytes
    from orb_slam3_modified_amd.matcher import ORBmatcher, SearchTarget
    H, W, params = 480, 752, (1000, 1.2, 8, 20, 7)
    ex = ORBextractor(*params, device_id=0)
    cap = ex.capacity
    scale = np.ones(params[2], np.float32)
    for i in range(1, params[2]):
        scale[i] = np.float32(scale[i - 1] * np.float32(params[1]))
    inv = (np.float32(1.0) / (scale * scale)).astype(np.float32)
    res = {"frames": B, "capacity": cap, "neighbours": len(NEIGHBOURS), "path": "lds" if lds_bytes(cap) <= LDS_MAX else "global"}
    x = Extracted(ex, B, H, W, repeats)
    res["d_extract_batch_device_ms"] = x.extract_ms
    res["keypoints_per_frame_median"] = int(np.median(x.hc[:, 0]))
    s, dev = x.s, x.dev
    # (d)'s second half: the FeatureVector transform, as tools/trimatch_times.py measures it
    trainer, docs = ex.clone(), []
    for a in range(0, train_frames, 64):
        docs += [r[2] for r in trainer.extract_batch(synth.make_stream(64, 480, 640, 9000 + a), (0, 1000))]
    gv = ORBVocabulary(ex)
    gv.create(docs, 10, 6, 0, 0, seed=2024)
    bb = BowBatch(gv, 4)
    fv = bb.transform_device(x.desc, x.counts, B, cap, stream=s.cuda_stream, bow=False)
    res["d_transform_featurevectors_ms"] = timed(s, lambda: bb.transform_device(x.desc, x.counts, B, cap, out=fv, stream=s.cuda_stream, bow=False), repeats)
    bb.close()
    feed = res["d_extract_batch_device_ms"]["median"] + res["d_transform_featurevectors_ms"]["median"]

    parm = grid_parameters(0, 0, W, H)
    side = FuseSide(x.kps, x.desc, x.counts, torch.from_numpy(np.tile(parm, (B, 1))).to(dev), B, cap, None)
    pdesc = x.desc.view(-1, 32)
    fb = FuseBatch(0)
    fb.grids_device(side, stream=s.cuda_stream)
    res["g_grids_device_ms"] = timed(s, lambda: fb.grids_device(side, stream=s.cuda_stream), repeats)
    fq = [frame_queries(x, f, scale) for f in range(B)]
    lists = {}
    own = [(f, (f + j) % B) for f in range(B) for j in NEIGHBOURS]                     # (whose points, searched keyframe)
    q = np.zeros((len(own), cap), QUERY_DTYPE)
    q["point"] = -1
    for p, (f, _) in enumerate(own):
        q[p, :len(fq[f])] = fq[f]
    lists["own_into_neighbours"] = (q, np.array([len(fq[f]) for f, _ in own], np.int32), np.array([k for _, k in own], np.int32))
    q = np.zeros((B, len(NEIGHBOURS) * cap), QUERY_DTYPE)
    q["point"] = -1
    nq = np.zeros(B, np.int32)
    for f in range(B):
        row = np.concatenate([fq[(f + j) % B] for j in NEIGHBOURS])
        q[f, :len(row)], nq[f] = row, len(row)
    lists["neighbours_into_own"] = (q, nq, np.arange(B, dtype=np.int32))

    om = ORBmatcher(ex)
    grid = dict(min_x=parm[0], min_y=parm[1], inv_w=parm[2], inv_h=parm[3])
    targets = {}
    total_search = 0.0
    for name, (query, nquery, pairs) in lists.items():
        P, Q = query.shape
        tq = torch.from_numpy(query.view(np.uint8).reshape(P, Q, 32)).to(dev)
        tn, tp = torch.from_numpy(nquery).to(dev), torch.from_numpy(pairs).to(dev)
        torch.cuda.synchronize()
        r = res.setdefault(name, {"pairs": P, "qcap": Q, "queries": int(nquery.sum())})
        out = fb.search_device(side, tq, tn, tp, pdesc, inv, True, 50, stream=s.cuda_stream)
        r["s_search_device_ms"] = timed(s, lambda: fb.search_device(side, tq, tn, tp, pdesc, inv, True, 50, stream=s.cuda_stream, out=out), repeats)
        torch.cuda.synchronize()
        nf, bi, bd = out.nfound.cpu().numpy(), out.best_idx.cpu().numpy(), out.best_dist.cpu().numpy()
        assert (nf >= 0).all()
        r["found_per_pair_median"] = int(np.median(nf))
        r["queries_with_a_candidate"] = int((bi >= 0).sum())
        r["s_us_per_pair"] = round(1000.0 * r["s_search_device_ms"]["median"] / P, 4)
        total_search += r["s_search_device_ms"]["median"]
        # (a): the per-pair path on a sample of the same pairs
        ts = []
        for p in np.linspace(0, P - 1, min(sample, P)).astype(int):
            k, n = int(pairs[p]), int(nquery[p])
            if k not in targets:
                nk = int(x.hc[k, 0])
                targets[k] = SearchTarget(om, x.hk[k, :nk], x.hd[k, :nk], grid, np.full(nk, -1.0, np.float32), inv)
            qq = query[p, :n]
            qd = x.hd.reshape(-1, 32)[qq["point"]]
            targets[k].nearest(qq["x"], qq["y"], qq["r"], qq["min_level"], qq["max_level"], qd, qq["ur"])       # warm
            t0 = time.perf_counter()
            wi, wd = targets[k].nearest(qq["x"], qq["y"], qq["r"], qq["min_level"], qq["max_level"], qd, qq["ur"])
            ts.append((time.perf_counter() - t0) * 1e6)
            assert np.array_equal(wi, bi[p, :n]) and np.array_equal(wd, bd[p, :n]), (name, p)
        r["a_target_nearest_us_per_pair"] = stats(ts)
        r["a_over_s_per_pair"] = round(r["a_target_nearest_us_per_pair"]["median"] / r["s_us_per_pair"], 2)
        r["s_faster_per_pair_than_a"] = bool(r["s_us_per_pair"] < r["a_target_nearest_us_per_pair"]["min"])
        del tq, out
    for t in targets.values():
        t.close()
    fb.close()
    batch = res["g_grids_device_ms"]["median"] + total_search
    res["search_in_neighbors_per_keyframe_us"] = round(1000.0 * batch / B, 3)
    res["extraction_plus_transform_per_keyframe_us"] = round(1000.0 * feed / B, 3)
    res["batch_over_extraction_plus_transform"] = round(batch / feed, 4)
    res["batch_below_extraction_plus_transform"] = bool(batch < feed)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--train-frames", type=int, default=128, help="480 x 640 frames whose descriptors train the tree of (d)")
    ap.add_argument("--sample", type=int, default=128, help="pairs of each list that the per-pair path (a) is timed on")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    assert args.repeats >= 10
    from orb_slam3_modified_amd import build
    out = {"stamp": build.stamp(), "repeats": args.repeats}
    out["euroc_752x480_1000"] = run(args.frames, args.repeats, args.train_frames, args.sample)
    write_result(args.out, "tools/fuse_times.py: batched Fuse search, HIP-event medians [min, max] of --repeats runs (ms)", out)


if __name__ == "__main__":
    main()
