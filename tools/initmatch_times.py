#!/usr/bin/env python3
"""Batched SearchForInitialization times (liborbx_initmatch.so) -> profiles/initmatch_times_r10.txt.

256 synthetic frames at the EuRoC shape (752 x 480; 1000 features, 1.2, 8 levels, 20 / 7) resident in HBM, window 100, nn_ratio 0.9, the
rotation filter on, the window centres F1's own keypoints.  Two pair lists: 256 pairs (f, f + 1) and 2560 pairs (every frame against the ten
that follow it), frame indices modulo 256.  Per list:
  (a) orbx_initmatch_pairs_device, HIP events on one stream, `--repeats` runs after three warm-up runs: median [min, max]
  (b) the loop of orbx_search_for_initialization over the same pairs from host copies, the only way before this library (wall clock, C calls
      only); the batched results are checked against its results in the same run
  (c) the oracle's SearchForInitialization on one core (wall clock, one run)
  (d) the batch extraction that feeds (a), HIP events
  split: (a) once more on a timing build of the same source without phase B (-DORBX_INITMATCH_NO_CHAIN): what is left is the parallel part,
      the difference is the sequential core
and (a), (b) for 32 pairs of the initialisation extractor's frames (640 x 480, 5000 features): the global-memory path, the longest chain.
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from times_util import Extracted, pair_lists, stats, timed, write_result  # noqa: E402
OUT = os.path.join(ROOT, "profiles", "initmatch_times_r10.txt")


def no_chain_library():
    """The timing build: the library's one source with phase B compiled out, beside the objects of the in-tree build."""
    from orb_slam3_modified_amd import _lib, build
    src = os.path.join(build.CSRC, build.INITMATCH_SOURCE)
    out = os.path.join(os.path.dirname(build.OUT), "build", "liborbx_initmatch_nochain.so")
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        flags = [f for f in build.FLAGS if f != "-ldl"] + ["-fvisibility=hidden", "-DORBX_INITMATCH_NO_CHAIN"]
        subprocess.check_call([os.environ.get("HIPCC", "hipcc")] + flags + [src, "-o", out, "-L", os.path.dirname(build.OUT),
                                                                            "-l:" + os.path.basename(build.OUT), "-Wl,-rpath," + os.path.dirname(build.OUT), "-ldl"])
    return _lib.initmatch_lib(out)


def run(shape, params, B, lists, repeats, oracle, split):
    import torch
    from orb_slam3_modified_amd import ORBextractor, _lib
    from orb_slam3_modified_amd._lib import ptr
    from orb_slam3_modified_amd.initmatch import LDS_MAX, InitMatchBatch, InitSide, lds_bytes
    H, W = shape
    window, ratio, bounds = 100, 0.9, (0.0, 0.0, float(W), float(H))
    ex = ORBextractor(*params, device_id=0)
    cap = ex.capacity
    x = Extracted(ex, B, H, W, repeats)
    s, dev, kps, desc, counts, hk, hd, hc = x.s, x.dev, x.kps, x.desc, x.counts, x.hk, x.hd, x.hc
    res = {"frames": B, "capacity": cap, "window": window, "nn_ratio": ratio, "path": "lds" if lds_bytes(cap, cap) <= LDS_MAX else "global"}
    res["d_extract_batch_device_ms"] = x.extract_ms
    host = [(np.ascontiguousarray(hk[f, :hc[f, 0]]), np.ascontiguousarray(hd[f, :hc[f, 0]])) for f in range(B)]
    res["keypoints_per_frame_median"] = int(np.median(hc[:, 0]))
    res["level0_per_frame_median"] = int(np.median([(k["octave"] == 0).sum() for k, _ in host]))
    side = InitSide(kps, desc, counts, B, cap)
    L = _lib.lib()
    mb = InitMatchBatch(0)
    nc = InitMatchBatch(0, library=no_chain_library()) if split else None
    for name, pairs in lists.items():
        tp = torch.from_numpy(pairs).to(dev)
        torch.cuda.synchronize()
        out = mb.pairs_device(side, side, tp, bounds, window, ratio, True, stream=s.cuda_stream)
        r = res.setdefault(name, {})
        r["a_batched_device_call_ms"] = timed(s, lambda: mb.pairs_device(side, side, tp, bounds, window, ratio, True, stream=s.cuda_stream, out=out), repeats)
        r["a_over_d"] = round(r["a_batched_device_call_ms"]["median"] / res["d_extract_batch_device_ms"]["median"], 4)
        torch.cuda.synchronize()
        gn, g12 = out.nmatches.cpu().numpy(), out.matches12.cpu().numpy()
        r["matches_per_pair_median"] = int(np.median(gn))
        if nc is not None:
            o2 = nc.pairs_device(side, side, tp, bounds, window, ratio, True, stream=s.cuda_stream)
            r["split_without_phase_b_ms"] = timed(s, lambda: nc.pairs_device(side, side, tp, bounds, window, ratio, True, stream=s.cuda_stream, out=o2), repeats)
            r["split_chain_share_of_a"] = round(1.0 - r["split_without_phase_b_ms"]["median"] / r["a_batched_device_call_ms"]["median"], 3)
        # (b) the per-pair loop of before
        m12, n_ = np.zeros(cap, np.int32), C.c_int(0)
        ts = []
        for rep in range(4 if len(pairs) <= 256 else 3):
            t0 = time.perf_counter()
            for i, (ia, ib) in enumerate(pairs.tolist()):
                (k1, d1), (k2, d2) = host[ia], host[ib]
                prev = np.stack([k1["x"], k1["y"]], 1).astype(np.float32)
                _lib.check(L.orbx_search_for_initialization(ex._ctx, ptr(k1), ptr(d1), len(k1), ptr(k2), ptr(d2), len(k2), *bounds, ptr(prev), window,
                                                            ratio, 1, ptr(m12), C.byref(n_)), ex._ctx)
                if rep == 0:
                    assert n_.value == gn[i] and np.array_equal(m12[:len(k1)], g12[i, :len(k1)]), ("batched != orbx_search_for_initialization", name, i)
            ts.append((time.perf_counter() - t0) * 1e3)
        r["b_orbx_search_for_initialization_loop_ms"] = stats(ts[1:])
        r["b_fastest_over_a_slowest"] = round(r["b_orbx_search_for_initialization_loop_ms"]["min"] / r["a_batched_device_call_ms"]["max"], 1)
        if oracle:
            from oracle import pyoracle as po
            t0 = time.perf_counter()
            for ia, ib in pairs.tolist():
                (k1, d1), (k2, d2) = host[ia], host[ib]
                po.search_for_initialization(k1, d1, k2, d2, bounds, np.stack([k1["x"], k1["y"]], 1), window, ratio, True)
            r["c_oracle_one_core_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    mb.close()
    if nc is not None:
        nc.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--no-split", action="store_true")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    assert args.repeats >= 10
    from orb_slam3_modified_amd import build
    B = args.frames
    out = {"stamp": build.stamp(), "repeats": args.repeats}
    out["euroc_752x480_1000"] = run((480, 752), (1000, 1.2, 8, 20, 7), B, pair_lists(B), args.repeats, not args.no_oracle, not args.no_split)
    out["vga_640x480_5000"] = run((480, 640), (5000, 1.2, 8, 20, 7), 33, {"32_pairs_f_f1": np.array([(f, f + 1) for f in range(32)], np.int32)},
                                  args.repeats, not args.no_oracle, not args.no_split)
    write_result(args.out, "tools/initmatch_times.py: batched SearchForInitialization, HIP-event medians [min, max] of --repeats runs (ms); (b), (c): wall clock", out)


if __name__ == "__main__":
    main()
