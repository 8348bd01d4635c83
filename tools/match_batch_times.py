#!/usr/bin/env python3
"""Batched SearchByBoW times (liborbx_match.so) -> profiles/match_batch_times_r9.txt.

256 synthetic frames at the EuRoC shape (752 x 480; 1000 features, 1.2, 8 levels, 20 / 7) resident in HBM, a k = 10, L = 6 tree
(ORBVocabulary.create), levelsup 4, nn_ratio 0.7, the rotation filter on.  Two pair lists: 256 pairs (f, f + 1) and 2560 pairs (every frame
against the ten that follow it), frame indices modulo 256.  Per list:
  (a) orbx_match_bow_pairs_device, HIP events on one stream, `--repeats` runs after three warm-up runs: median [min, max]
  (b) the loop of orbx_search_by_bow over the same pairs from host copies, the only way before this library (wall clock, C calls only)
  (c) the oracle's SearchByBoW on one core (wall clock, one run)
  (d) the batch extraction and the FeatureVector transform that feed (a), HIP events
and (a), (b) once more for levelsup = L: one node, every feature against every feature.  The batched results are checked against (b)'s.
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from times_util import Extracted, pair_lists, stats, timed, write_result  # noqa: E402
OUT = os.path.join(ROOT, "profiles", "match_batch_times_r9.txt")


def csr(fv):
    nodes = sorted(fv)
    p, idx = [0], []
    for k in nodes:
        idx.extend(fv[k])
        p.append(len(idx))
    return np.array(nodes, np.uint32), np.array(p, np.int32), np.array(idx, np.uint32)


def run(B, repeats, train_frames, oracle):
    import torch
    from orb_slam3_modified_amd import ORBextractor, ORBVocabulary, _lib, synth
    from orb_slam3_modified_amd._lib import ptr
    from orb_slam3_modified_amd.bow import BowBatch
    from orb_slam3_modified_amd.match import FRAME, MatchBatch, MatchSide
    H, W, params, ratio = 480, 752, (1000, 1.2, 8, 20, 7), 0.7
    ex = ORBextractor(*params, device_id=0)
    cap = ex.capacity
    trainer, docs = ex.clone(), []
    for a in range(0, train_frames, 64):
        docs += [r[2] for r in trainer.extract_batch(synth.make_stream(64, 480, 640, 9000 + a), (0, 1000))]
    gv = ORBVocabulary(ex)
    gv.create(docs, 10, 6, 0, 0, seed=2024)
    res = {"frames": B, "capacity": cap, "nn_ratio": ratio, "training_descriptors": int(sum(len(d) for d in docs)), "tree": gv.info()}
    L = _lib.lib()
    mb = MatchBatch(0)
    x = Extracted(ex, B, H, W, repeats)
    res["d_extract_batch_device_ms"] = x.extract_ms
    s, dev, kps, desc, counts, hk, hd, hc = x.s, x.dev, x.kps, x.desc, x.counts, x.hk, x.hd, x.hc
    lists = pair_lists(B)
    for levelsup, names in ((4, list(lists)), (6, ["256_pairs_f_f1"])):
        bb = BowBatch(gv, levelsup)
        fv = bb.transform_device(desc, counts, B, cap, stream=s.cuda_stream, bow=False)
        leg = res.setdefault(f"levelsup_{levelsup}", {})
        leg["d_transform_featurevectors_ms"] = timed(s, lambda: bb.transform_device(desc, counts, B, cap, out=fv, stream=s.cuda_stream, bow=False), repeats)
        side = MatchSide.of(kps, desc, counts, fv, B, cap)
        fn, fp, ff, fc = (fv.fv_node.cpu().numpy().view(np.uint32), fv.fv_ptr.cpu().numpy(), fv.fv_feat.cpu().numpy().view(np.uint32), fv.fv_n.cpu().numpy())
        hfv = [{int(fn[f, j]): ff[f, fp[f, j]:fp[f, j + 1]].astype(np.int64).tolist() for j in range(int(fc[f]))} for f in range(B)]
        leg["fv_nodes_per_frame_median"] = int(np.median(fc))
        host = []
        for f in range(B):
            n = int(hc[f, 0])
            host.append((np.ascontiguousarray(hd[f, :n]), np.ascontiguousarray(hk[f, :n]["angle"]), np.ones(n, np.uint8)) + csr(hfv[f]))
        for name in names:
            pairs = lists[name]
            tp = torch.from_numpy(pairs).to(dev)
            out = mb.bow_pairs_device(side, side, tp, FRAME, ratio, True, stream=s.cuda_stream)
            r = leg.setdefault(name, {})
            r["a_batched_device_call_ms"] = timed(s, lambda: mb.bow_pairs_device(side, side, tp, FRAME, ratio, True, stream=s.cuda_stream, out=out), repeats)
            torch.cuda.synchronize()
            gn, gb2a = out.nmatches.cpu().numpy(), out.b2a.cpu().numpy()
            r["matches_per_pair_median"] = int(np.median(gn))
            # (b) the per-pair loop of before
            match, n_ = np.zeros(cap, np.int32), C.c_int(0)
            ts = []
            for rep in range(5 if len(pairs) <= 256 and levelsup == 4 else 3):
                t0 = time.perf_counter()
                for i, (ia, ib) in enumerate(pairs.tolist()):
                    kd, ka, kv, kn, kp_, ki = host[ia]
                    fd, fa, _, fn_, fp_, fi = host[ib]
                    _lib.check(L.orbx_search_by_bow(ex._ctx, ptr(kd), ptr(ka), ptr(kv), len(kd), ptr(kn), ptr(kp_), ptr(ki), len(kn), ptr(fd), ptr(fa), len(fd),
                                                    ptr(fn_), ptr(fp_), ptr(fi), len(fn_), ratio, 1, ptr(match), C.byref(n_)), ex._ctx)
                    if rep == 0:
                        assert n_.value == gn[i] and np.array_equal(match[:len(fd)], gb2a[i, :len(fd)]), ("batched != orbx_search_by_bow", name, i)
                ts.append((time.perf_counter() - t0) * 1e3)
            r["b_orbx_search_by_bow_loop_ms"] = stats(ts[1:])
            r["b_fastest_over_a_slowest"] = round(r["b_orbx_search_by_bow_loop_ms"]["min"] / r["a_batched_device_call_ms"]["max"], 1)
            if oracle and levelsup == 4:
                from oracle import pyoracle as po
                t0 = time.perf_counter()
                for ia, ib in pairs.tolist():
                    po.search_by_bow(host[ia][0], host[ia][1], host[ia][2], hfv[ia], host[ib][0], host[ib][1], hfv[ib], ratio, True)
                r["c_oracle_one_core_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        bb.close()
    mb.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--train-frames", type=int, default=128, help="480 x 640 frames whose descriptors train the tree")
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    assert args.repeats >= 10
    from orb_slam3_modified_amd import build
    out = {"stamp": build.stamp(), "repeats": args.repeats}
    out["euroc_752x480"] = run(args.frames, args.repeats, args.train_frames, not args.no_oracle)
    write_result(args.out, "tools/match_batch_times.py: batched SearchByBoW, HIP-event medians [min, max] of --repeats runs (ms); (b), (c): wall clock", out)


if __name__ == "__main__":
    main()
