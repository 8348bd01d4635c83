#!/usr/bin/env python3
"""Batched SearchForTriangulation times (liborbx_trimatch.so) -> profiles/trimatch_times_r11.txt.

256 synthetic frames at the EuRoC shape (752 x 480; 1000 features, 1.2, 8 levels, 20 / 7) resident in HBM, a k 10 / L 6 vocabulary trained
on the device (ORBVocabulary.create), the rotation filter on, monocular, no feature with a point, every pair with the fundamental matrix of a
sideways translation under EuRoC's intrinsics (the synthetic camera moves 1.5 px right and 0.5 px down per frame).  Two pair lists: 256 pairs
(f, f + 1) and 2560 pairs (every frame against the ten that follow it, what LocalMapping::CreateNewMapPoints asks for), frame indices modulo
256.  Per levelsup (4, and 6 = L: one node, every feature against every feature) and list:
  (a) orbx_trimatch_pairs_device, HIP events on one stream, `--repeats` runs after three warm-up runs: median [min, max]
  (m) k_match_pairs (orbx_match_bow_pairs_device, frame mode, ratio 0.7) on the same pairs, for comparison: one wave per node there
  (d) the batch extraction and the FeatureVector transform that feed (a), HIP events
The condition to check: (a) for 2560 pairs stays below (d) extraction + transform of the 256 frames in the same run.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from times_util import Extracted, pair_lists, timed, write_result  # noqa: E402
OUT = os.path.join(ROOT, "profiles", "trimatch_times_r11.txt")
EUROC_K = np.array([[458.654, 0.0, 367.215], [0.0, 457.296, 248.375], [0.0, 0.0, 1.0]])


def run(B, repeats, train_frames):
    import torch
    from orb_slam3_modified_amd import ORBextractor, ORBVocabulary, synth
    from orb_slam3_modified_amd.bow import BowBatch
    from orb_slam3_modified_amd.match import FRAME, MatchBatch, MatchSide
    from orb_slam3_modified_amd.trimatch import LDS_MAX, TriMatchBatch, TriMatchSide, fundamental, geometry, lds_bytes
    H, W, params = 480, 752, (1000, 1.2, 8, 20, 7)
    ex = ORBextractor(*params, device_id=0)
    cap = ex.capacity
    trainer, docs = ex.clone(), []
    for a in range(0, train_frames, 64):
        docs += [r[2] for r in trainer.extract_batch(synth.make_stream(64, 480, 640, 9000 + a), (0, 1000))]
    gv = ORBVocabulary(ex)
    gv.create(docs, 10, 6, 0, 0, seed=2024)
    scale = np.ones(params[2], np.float32)
    for i in range(1, params[2]):
        scale[i] = np.float32(scale[i - 1] * np.float32(params[1]))
    sigma2 = (scale * scale).astype(np.float32)
    row = geometry(fundamental(EUROC_K, np.eye(3), [1.0, 0.0, 0.0], EUROC_K), (np.inf, np.nan))
    res = {"frames": B, "capacity": cap, "tree": gv.info(), "path": "lds" if lds_bytes(cap, cap) <= LDS_MAX else "global"}
    tb, mb = TriMatchBatch(0), MatchBatch(0)
    x = Extracted(ex, B, H, W, repeats)
    res["d_extract_batch_device_ms"] = x.extract_ms
    res["keypoints_per_frame_median"] = int(np.median(x.hc[:, 0]))
    s, dev, kps, desc, counts = x.s, x.dev, x.kps, x.desc, x.counts
    lists = pair_lists(B)
    for levelsup in (4, 6):
        bb = BowBatch(gv, levelsup)
        fv = bb.transform_device(desc, counts, B, cap, stream=s.cuda_stream, bow=False)
        leg = res.setdefault(f"levelsup_{levelsup}", {})
        leg["d_transform_featurevectors_ms"] = timed(s, lambda: bb.transform_device(desc, counts, B, cap, out=fv, stream=s.cuda_stream, bow=False), repeats)
        leg["fv_nodes_per_frame_median"] = int(np.median(fv.fv_n.cpu().numpy()))
        feed = res["d_extract_batch_device_ms"]["median"] + leg["d_transform_featurevectors_ms"]["median"]
        tside, mside = TriMatchSide.of(kps, desc, counts, fv, B, cap), MatchSide.of(kps, desc, counts, fv, B, cap)
        for name, pairs in lists.items():
            tp = torch.from_numpy(pairs).to(dev)
            tg = torch.from_numpy(np.tile(row, (len(pairs), 1))).to(dev)
            torch.cuda.synchronize()
            r = leg.setdefault(name, {})
            out = tb.pairs_device(tside, tside, tp, tg, scale, sigma2, stream=s.cuda_stream)
            r["a_batched_device_call_ms"] = timed(s, lambda: tb.pairs_device(tside, tside, tp, tg, scale, sigma2, stream=s.cuda_stream, out=out), repeats)
            torch.cuda.synchronize()
            gn = out.nmatches.cpu().numpy()
            assert (gn >= 0).all()
            r["matches_per_pair_median"] = int(np.median(gn))
            r["a_over_extraction_plus_transform"] = round(r["a_batched_device_call_ms"]["median"] / feed, 4)
            r["a_slowest_below_extraction_plus_transform"] = bool(r["a_batched_device_call_ms"]["max"] < feed)
            mo = mb.bow_pairs_device(mside, mside, tp, FRAME, 0.7, True, stream=s.cuda_stream)
            r["m_k_match_pairs_ms"] = timed(s, lambda: mb.bow_pairs_device(mside, mside, tp, FRAME, 0.7, True, stream=s.cuda_stream, out=mo), repeats)
        bb.close()
    tb.close()
    mb.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--train-frames", type=int, default=128, help="480 x 640 frames whose descriptors train the tree")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    assert args.repeats >= 10
    from orb_slam3_modified_amd import build
    out = {"stamp": build.stamp(), "repeats": args.repeats}
    out["euroc_752x480_1000"] = run(args.frames, args.repeats, args.train_frames)
    write_result(args.out, "tools/trimatch_times.py: batched SearchForTriangulation, HIP-event medians [min, max] of --repeats runs (ms)", out)


if __name__ == "__main__":
    main()
