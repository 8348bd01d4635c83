#!/usr/bin/env python3
"""Batched two-camera rig SearchByBoW times (liborbx_rigbow.so) -> profiles/rigbow_times_r25.txt.

  python tools/rigbow_times.py [--frames 256] [--features 1500] [--repeats 15] [--passes 3] [--out PATH]

The shape: `--frames` TUM-VI-shaped rig frames, SYNTHETIC: `--features` keypoints a side at capacity `--features`, descriptors that drift
by a few bits from frame to frame and between the cameras, random angles that drift by a few degrees; every frame against its
predecessor as keyframe (`--frames` pairs), 70 % of the keyframe's features valid, nn_ratio 0.7, the rotation filter on.  The vocabulary
(10 branches, 6 levels) is trained on the device on the first frames' descriptors.  At levelsup 4 and levelsup = L (one node):
  stack       orbx_rigbow_stack_device, HIP events on one stream, `--repeats` runs after three warm-up runs: median [min, max]
  transform   BowBatch.transform_device on the stacked buffers (FeatureVectors only)
  rig_bow     orbx_rigbow_pairs_device, frame mode, and which path (LDS or global) the shape took
  left_bow    MatchBatch.bow_pairs_device on the LEFT sides alone (their own FeatureVectors): what the second camera costs
  adapter     the per-pair loop through the drop-in adapter's rig SearchByBoW (csrc/ref_adapter/ORBmatcher.cc over liborbx.so) on the same
              frames and FeatureVectors (tools/rigbow_adapter_loop.cpp): wall clock around the matcher calls alone, summed over the pairs,
              median [min, max] of `--passes` passes; the two paths' results are compared slot by slot (adapter_equal)."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from rigmatch_times import write_records  # noqa: E402
from times_util import stats, timed, write_result  # noqa: E402
OUT = os.path.join(ROOT, "profiles", "rigbow_times_r25.txt")
SIZE = 512


def adapter_loop_path():
    """tools/rigbow_adapter_loop.cpp over the drop-in adapter and liborbx.so, beside the objects of the in-tree build."""
    from orb_slam3_modified_amd import build
    from tests import world_util as wu
    build.build()
    src = os.path.join(ROOT, "tools", "rigbow_adapter_loop.cpp")
    out = os.path.join(os.path.dirname(build.OUT), "build", "rigbow_adapter_loop.bin")
    if wu._stale(out, wu._deps() + [src, os.path.join(wu.PKG, "liborbx.so")]):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++"] + wu.CXXFLAGS + wu.INCLUDES + ["-I", wu.SUP, src, wu.ADAPTER_SRC, "-o", out, "-DORBX_NO_CV_CALIBRATION", "-L", wu.PKG,
                               "-lorbx", "-Wl,-rpath," + wu.PKG, "-Wl,--allow-shlib-undefined"])
    return out


def make_frames(rng, F, n):
    """kps / desc / counts per camera: a base set of n descriptors, each frame and camera a few flipped bits away from it."""
    from orb_slam3_modified_amd._lib import KP_DTYPE
    base, angle = rng.integers(0, 256, (n, 32)).astype(np.uint8), rng.uniform(0, 340, n)
    out = {}
    for cam in "lr":
        d = np.tile(base, (F, 1, 1))
        for _ in range(6):                                       # six random single-bit flips a descriptor
            byte, bit = rng.integers(0, 32, (F, n, 1)), rng.integers(0, 8, (F, n, 1))
            np.put_along_axis(d, byte, np.take_along_axis(d, byte, 2) ^ (1 << bit).astype(np.uint8), 2)
        k = np.zeros((F, n), KP_DTYPE)
        k["x"], k["y"], k["size"], k["octave"] = rng.uniform(1, SIZE - 2, (F, n)), rng.uniform(1, SIZE - 2, (F, n)), 31.0, rng.integers(0, 8, (F, n))
        k["angle"] = angle[None] + rng.normal(0, 4.0, (F, n)) + 10.0
        perm = np.stack([rng.permutation(n) for _ in range(F)])   # a frame's features in an order of its own
        out["kps_" + cam], out["desc_" + cam] = np.take_along_axis(k, perm, 1), np.take_along_axis(d, perm[..., None], 1)
        out["counts_" + cam] = np.tile(np.array([[n, 0]], np.int32), (F, 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--features", type=int, default=1500)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--passes", type=int, default=3, help="passes of the adapter loop")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--build-only", action="store_true", help="build the adapter loop and stop (no device is touched)")
    args = ap.parse_args()
    adapter = adapter_loop_path()
    if args.build_only:
        return
    import torch
    from orb_slam3_modified_amd import ORBextractor, ORBVocabulary, build
    from orb_slam3_modified_amd.bow import BowBatch
    from orb_slam3_modified_amd.match import MatchBatch, MatchSide
    from orb_slam3_modified_amd.rigbow import FRAME, LDS_MAX, RigBowBatch, RigBowSide, lds_bytes
    from tests.rigmatch_world import read_dump
    F, n, ratio = args.frames, args.features, 0.7
    cap = 2 * n
    rng = np.random.default_rng(25)
    h = make_frames(rng, F, n)
    hvalid = (rng.random((F, cap)) < 0.7).astype(np.uint8)
    pairs = np.array([((f + F - 1) % F, f) for f in range(F)], np.int32)
    dev = torch.device("cuda", 0)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (-1,)) if a.dtype.names else np.ascontiguousarray(a)).to(dev)   # noqa: E731
    t = {k: to(v) for k, v in h.items()}
    valid, d_pairs = to(hvalid), to(pairs)
    ex = ORBextractor(1000, 1.2, 8, 20, 7, device_id=0)
    gv = ORBVocabulary(ex)
    gv.create([h["desc_l"][f] for f in range(min(F, 16))], 10, 6, 0, 0, seed=2025)
    stream = torch.cuda.Stream(device=dev)
    rb, mb = RigBowBatch(0), MatchBatch(0)
    limit = max(0, min(LDS_MAX, int(os.environ.get("ORBX_RIGBOW_LDS", LDS_MAX))))   # what orbx_rigbow_create reads
    res = {"stamp": build.stamp(), "shape": {"frames": F, "pairs": len(pairs), "features_per_side": n, "stacked_capacity": cap, "frames_are": "synthetic"},
           "nn_ratio": ratio, "tree": gv.info(), "lds_bytes_needed": lds_bytes(cap, cap), "lds_limit": limit,
           "path": "lds" if lds_bytes(cap, cap) <= limit and cap <= 65535 else "global"}
    torch.cuda.synchronize()
    st = rb.stack_device(t["kps_l"], t["desc_l"], t["counts_l"], t["kps_r"], t["desc_r"], t["counts_r"], stream=stream.cuda_stream)
    res["stack_ms"] = timed(stream, lambda: rb.stack_device(t["kps_l"], t["desc_l"], t["counts_l"], t["kps_r"], t["desc_r"], t["counts_r"],
                                                            stream=stream.cuda_stream, out=st), args.repeats)
    for levelsup in (4, 6):
        leg = res.setdefault("levelsup_%d" % levelsup, {})
        bb = BowBatch(gv, levelsup)
        fv = bb.transform_device(st.desc, st.counts, F, cap, stream=stream.cuda_stream, bow=False)
        leg["transform_ms"] = timed(stream, lambda: bb.transform_device(st.desc, st.counts, F, cap, stream=stream.cuda_stream, bow=False, out=fv), args.repeats)
        fvl = bb.transform_device(t["desc_l"], t["counts_l"], F, n, stream=stream.cuda_stream, bow=False)
        a, b = RigBowSide.of(st, fv, valid), RigBowSide.of(st, fv)
        out = rb.bow_pairs_device(a, b, d_pairs, FRAME, ratio, True, stream=stream.cuda_stream)
        leg["rig_bow_ms"] = timed(stream, lambda: rb.bow_pairs_device(a, b, d_pairs, FRAME, ratio, True, stream=stream.cuda_stream, out=out), args.repeats)
        la = MatchSide.of(t["kps_l"], t["desc_l"], t["counts_l"], fvl, F, n, valid[:, :n].contiguous())
        lb = MatchSide.of(t["kps_l"], t["desc_l"], t["counts_l"], fvl, F, n)
        lout = mb.bow_pairs_device(la, lb, d_pairs, FRAME, ratio, True, stream=stream.cuda_stream)
        leg["left_bow_ms"] = timed(stream, lambda: mb.bow_pairs_device(la, lb, d_pairs, FRAME, ratio, True, stream=stream.cuda_stream, out=lout), args.repeats)
        stream.synchronize()
        nm, b2a, a2b = out.nmatches.cpu().numpy(), out.b2a.cpu().numpy(), out.a2b.cpu().numpy()
        assert (nm >= 0).all()
        leg["matches_per_pair_median"] = int(np.median(nm))
        leg["left_matches_per_pair_median"] = int(np.median(lout.nmatches.cpu().numpy()))
        leg["keyframe_features_with_two_slots"] = int(((a2b >= 0).sum(2) == 2).sum())
        leg["common_nodes_first_pair"] = int(len(np.intersect1d(fv.fv_node[pairs[0, 0], :int(fv.fv_n[pairs[0, 0]])].cpu().numpy(),
                                                                fv.fv_node[pairs[0, 1], :int(fv.fv_n[pairs[0, 1]])].cpu().numpy())))
        leg["rig_over_left"] = round(leg["rig_bow_ms"]["median"] / leg["left_bow_ms"]["median"], 2)
        # the adapter's per-pair loop on the same frames and FeatureVectors, in a process of its own
        with tempfile.TemporaryDirectory() as tmp:
            inp, outp = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
            write_records(inp, {"shape": np.array([F, n, len(pairs), SIZE], np.int32), "call": np.array([ratio], np.float32), "pairs": pairs,
                                "kps_l": h["kps_l"].view(np.uint8), "kps_r": h["kps_r"].view(np.uint8), "desc_l": h["desc_l"], "desc_r": h["desc_r"],
                                "valid": hvalid, "fv_node": fv.fv_node.cpu().numpy().astype(np.int32), "fv_ptr": fv.fv_ptr.cpu().numpy().astype(np.int32),
                                "fv_feat": fv.fv_feat.cpu().numpy().astype(np.int32), "fv_n": fv.fv_n.cpu().numpy().astype(np.int32)})
            subprocess.run([adapter, inp, outp, str(args.passes)], check=True, timeout=1500)
            ad = read_dump(outp)
        leg["adapter_ms"] = stats(ad["ms"])
        leg["adapter_equal"] = bool(np.array_equal(ad["ids"].reshape(len(pairs), cap), b2a) and np.array_equal(ad["ret"], nm))
        leg["adapter_over_rig"] = round(leg["adapter_ms"]["median"] / leg["rig_bow_ms"]["median"], 2)
        bb.close()
    rb.close()
    mb.close()
    write_result(args.out, "tools/rigbow_times.py: stacked rig frames and the batched rig SearchByBoW, HIP-event medians [min, max] of --repeats runs (ms)", res)


if __name__ == "__main__":
    main()
