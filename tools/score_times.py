#!/usr/bin/env python3
"""Score-matrix times (liborbx_score.so) -> profiles/score_times_r14.txt.

The shape and the vocabulary of tools/bow_batch_times.py (c): 256 synthetic frames at the EuRoC shape (752 x 480; 1000 features, 1.2, 8
levels, 20 / 7), a k = 10, L = 6 tree trained on > 10^6 descriptors, their BowVectors resident in HBM; 256 x 256 (the batch against itself)
and 256 x 4096 (against the batch repeated).  One process, one stream; every variant is timed once per round, `--repeats` rounds after
three warm-up rounds (the variants interleaved, so that clock drift hits all of them alike); HIP-event median and [min, max] per variant:
  bow_l1      orbx_bow_score_matrix_device, the yardstick of the L1 form, on the same vectors in the same rounds
  score_<s>   orbx_score_matrix_device under each of the five device scorings
  score_L1_NORM_lds0   the L1 form with ORBX_SCORE_LDS=0: every query read where it lies
The L1 matrices of the two libraries are compared bit for bit before anything is timed.  The measuring runs in a child process under a time
limit (--limit seconds); the parent opens no GPU."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from times_util import stats, write_result  # noqa: E402
OUT = os.path.join(ROOT, "profiles", "score_times_r14.txt")
NAMES = {0: "L1_NORM", 1: "L2_NORM", 2: "CHI_SQUARE", 4: "BHATTACHARYYA", 5: "DOT_PRODUCT"}


def clocks():
    """The GPU's clock state as the driver reports it (read only)."""
    try:
        out = subprocess.run(["rocm-smi", "-d", "0", "--showclocks", "--showperflevel"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                             timeout=30).stdout
        return [l.strip() for l in out.splitlines() if "GPU[0]" in l and ("sclk" in l or "mclk" in l or "Performance" in l)]
    except Exception as e:   # noqa: BLE001
        return [f"not read: {e}"]


def interleaved(stream, variants, rounds):
    """variants: name -> fn.  HIP events around each fn() on `stream`, one run of every variant a round."""
    import torch
    ts = {k: [] for k in variants}
    for r in range(rounds + 3):
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if r >= 3:
                ts[k].append(e0.elapsed_time(e1))
    return {k: stats(v) for k, v in ts.items()}


def run(B, repeats, train_frames):
    import torch
    from orb_slam3_modified_amd import ORBextractor, ORBVocabulary, synth
    from orb_slam3_modified_amd.bow import BowBatch
    from orb_slam3_modified_amd.score import DEVICE_SCORINGS, ScoreBatch
    H, W, params, levelsup = 480, 752, (1000, 1.2, 8, 20, 7), 4
    ex = ORBextractor(*params, device_id=0)
    cap = ex.capacity
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    t = torch.from_numpy(synth.make_stream(B, H, W)).to(dev)
    z = lambda *shape, dt=torch.uint8: torch.zeros(shape, dtype=dt, device=dev)   # noqa: E731
    kps, desc, counts = z(B, cap, 28), z(B, cap, 32), z(B, 2, dt=torch.int32)
    trainer, docs = ex.clone(), []
    for a in range(0, train_frames, 64):
        docs += [r[2] for r in trainer.extract_batch(synth.make_stream(64, 480, 640, 9000 + a), (0, 1000))]
    gv = ORBVocabulary(ex)
    gv.create(docs, 10, 6, 0, 0, seed=2024)
    torch.cuda.synchronize()
    ex.extract_batch_device(t.data_ptr(), B, H, W, W, H * W, kps.data_ptr(), desc.data_ptr(), counts.data_ptr(), (0, 1000), stream=s.cuda_stream)
    bb = BowBatch(gv, levelsup)
    out = bb.transform_device(desc, counts, B, cap, stream=s.cuda_stream)
    s.synchronize()
    res = {"frames": B, "capacity": cap, "training_descriptors": int(sum(len(d) for d in docs)), "tree": gv.info(),
           "bow_entries_per_frame_median": int(np.median(out.bow_n.cpu().numpy()))}
    sb = ScoreBatch(0)
    os.environ["ORBX_SCORE_LDS"] = "0"
    sb0 = ScoreBatch(0)
    del os.environ["ORBX_SCORE_LDS"]
    rep = 4096 // B
    sides = {"%dx%d" % (B, B): (out.bow_ids, out.bow_vals, out.bow_n),
             "%dx%d" % (B, B * rep): (out.bow_ids.repeat(rep, 1), out.bow_vals.repeat(rep, 1), out.bow_n.repeat(rep))}
    for shape, (di, dv, dn) in sides.items():
        ndb = int(dn.shape[0])
        buf = {k: z(B, ndb, dt=torch.float64) for k in ["bow_l1", "score_L1_NORM_lds0"] + ["score_" + NAMES[k] for k in DEVICE_SCORINGS]}
        q = (out.bow_ids, out.bow_vals, out.bow_n, B, cap, di, dv, dn, ndb, cap)
        variants = {"bow_l1": lambda: bb.score_matrix_device(*q, scores=buf["bow_l1"], stream=s.cuda_stream)}
        for k in DEVICE_SCORINGS:
            variants["score_" + NAMES[k]] = (lambda k=k: sb.matrix_device(k, *q, scores=buf["score_" + NAMES[k]], stream=s.cuda_stream))
        variants["score_L1_NORM_lds0"] = lambda: sb0.matrix_device(0, *q, scores=buf["score_L1_NORM_lds0"], stream=s.cuda_stream)
        for fn in variants.values():
            fn()
        s.synchronize()
        want = buf["bow_l1"].cpu().numpy().tobytes()
        assert buf["score_L1_NORM"].cpu().numpy().tobytes() == want and buf["score_L1_NORM_lds0"].cpu().numpy().tobytes() == want, "the L1 matrices differ"
        res[shape + "_ms"] = interleaved(s, variants, repeats)
    for h in (bb, sb, sb0):
        h.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--train-frames", type=int, default=1088, help="480 x 640 frames whose descriptors train the tree (1088 -> > 10^6)")
    ap.add_argument("--limit", type=int, default=540, help="seconds the measuring child may take")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(run(args.frames, args.repeats, args.train_frames)), flush=True)
        return 0
    from orb_slam3_modified_amd import build
    out = {"stamp": build.stamp(), "repeats": args.repeats, "clocks_before": clocks()}
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--frames", str(args.frames), "--repeats", str(args.repeats), "--train-frames",
           str(args.train_frames)]
    try:
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.limit)
    except subprocess.TimeoutExpired:
        print("the measuring step ran into its time limit of %d s; nothing written" % args.limit)
        return 124
    lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    if p.returncode != 0 or not lines:
        print(p.stdout[-4000:])
        print("the measuring step failed (exit %d); nothing written" % p.returncode)
        return p.returncode or 1
    out["euroc_752x480"] = json.loads(lines[-1][7:])
    out["clocks_after"] = clocks()
    write_result(args.out, "tools/score_times.py: score matrices under the five device scorings and the bow library's L1 form, interleaved "
                 "HIP-event medians [min, max] of --repeats rounds (ms)", out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
