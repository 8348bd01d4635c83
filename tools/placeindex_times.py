"""Times of place recognition through the device inverted file (liborbx_placeindex.so) on an MI355X -> profiles/placeindex_times_r20.txt.

Two databases, 256 queries each, stride 1024, N-best with ten excluded rows a query and relocalization:
  euroc   tools/place_times.py's own: 256 synthetic EuRoC-shaped frames extracted and transformed on the device under a k = 10, L = 6 tree
          trained on the device; their BowVectors are the queries and, round robin, the 2000 and 4096 keyframes.  Every row shares a word
          with every query: the unfavourable case for a file, whose work goes with the postings.
  sparse  4096 keyframes of 256 distinct synthetic scenes under a vocabulary of 10^6 words: every scene owns a pool of 3000 words of its
          own, a keyframe or a query holds 1000 of its scene's pool (BowVectors drawn directly, L1-normalised).  A query shares words with
          its scene's sixteen keyframes and with nobody else.
In one run, interleaved, HIP events, median [min, max] of --repeats rounds after three warm-up rounds:
  (d) PlaceBatch.query_device                  the parent's dense call on the same arrays: the yardstick
  (i) PlaceIndex.query_device, fully synced    at 4, 16 and 64 lanes per query word (ORBX_PLACEINDEX_GROUP; 16 is the default)
  (t) the same with a tail of 16 and 256 rows  (synced at D - tail)
  (s) PlaceIndex.sync_device                   the rebuild on its own
Every (i) and (t) result is compared equal with (d)'s, all arrays and the OUT scores, before anything is timed.  --trace runs the indexed
calls once more under `rocprofv3 --kernel-trace` (a run of its own, not timed by events) and reports each kernel group's share of the call."""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from score_times import clocks, interleaved  # noqa: E402
from times_util import stats, write_result  # noqa: E402
OUT = os.path.join(ROOT, "profiles", "placeindex_times_r20.txt")
GROUPS = (4, 16, 64)
TAILS = (16, 256)
CCAP, NCAND = 16, 3
STAGES = {"clear": ("fillBuffer",), "count": ("k_index_count",), "tail": ("k_index_tail",), "score": ("k_index_score",),
          "unchanged": ("k_place_check", "k_index_stale", "k_place_members", "k_place_scan", "k_place_select")}


def euroc_vectors(B, train_frames):
    """(ids, vals, n) device tensors [B, cap] of B extracted frames, the tree's word count and what describes the run."""
    import torch
    from orb_slam3_modified_amd import ORBextractor, ORBVocabulary, synth
    from orb_slam3_modified_amd.bow import BowBatch
    H, W, params, levelsup = 480, 752, (1000, 1.2, 8, 20, 7), 4
    ex = ORBextractor(*params, device_id=0)
    cap, dev = ex.capacity, torch.device("cuda:0")
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
    bow = bb.transform_device(desc, counts, B, cap, stream=s.cuda_stream)
    s.synchronize()
    out = (bow.bow_ids.clone(), bow.bow_vals.clone(), bow.bow_n.clone())
    info = {"stride": cap, "training_descriptors": int(sum(len(d) for d in docs)), "tree": gv.info(),
            "bow_entries_per_query_median": int(np.median(bow.bow_n.cpu().numpy()))}
    bb.close()
    return out, gv.info()["words"], info


def sparse_vectors(B, D, stride, n_words=1000000, pool=3000, entries=1000, seed=2026):
    """Host arrays: B queries and D keyframes, frame i of scene i % B; scene s owns the words [s * pool, (s + 1) * pool)."""
    rng = np.random.default_rng(seed)
    assert B * pool <= n_words and entries <= stride

    def draw(count):
        ids, vals = np.zeros((count, stride), np.uint32), np.zeros((count, stride), np.float64)
        for i in range(count):
            ids[i, :entries] = np.sort(rng.choice(pool, entries, replace=False)) + (i % B) * pool
            v = rng.integers(1, 9, entries).astype(np.float64)
            vals[i, :entries] = v / v.sum()
        return ids.view(np.int32), vals, np.full(count, entries, np.int32)
    return draw(B), draw(D), n_words


def postings_touched(q_ids, q_n, d_ids, d_n, n_words):
    """Per query, the postings its words own in the file of the whole database."""
    lens = np.bincount(np.concatenate([d_ids[d, :max(n, 0)] for d, n in enumerate(d_n)]).astype(np.int64), minlength=n_words)
    return [int(lens[q_ids[i, :max(n, 0)].astype(np.int64)].sum()) for i, n in enumerate(q_n)]


class World:
    """One database with its queries on the device, both kinds."""

    def __init__(self, name, q, d, n_words):
        import torch
        from orb_slam3_modified_amd import place as pl
        from tests import place_model as pm
        dev = torch.device("cuda:0")
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev) if isinstance(a, np.ndarray) else a   # noqa: E731
        (qi, qv, qn), (di, dv, dn) = [tuple(up(a) for a in side) for side in (q, d)]
        self.name, self.n_words, B, D = name, n_words, int(qn.shape[0]), int(dn.shape[0])
        self.B, self.D, stride = B, D, int(qi.shape[1])
        kf_map = (np.arange(D) % 5 == 4).astype(np.int32)
        cov = np.array([[r - k if r - k >= 0 else -1 for k in range(1, 11)] for r in range(D)], np.int32)
        ep, ei, ne = pl.exclusions([sorted((37 * i + 11 * k) % D for k in range(10)) for i in range(B)])
        self.db = pl.PlaceDb(di, dv, dn, up(kf_map), up(cov), up(np.zeros(D, np.float32)), D, stride)
        q_map = up(np.zeros(B, np.int32))
        self.qs = {pm.RELOC: pl.PlaceQueries(qi, qv, qn, q_map, B, stride), pm.NBEST: pl.PlaceQueries(qi, qv, qn, q_map, B, stride, up(ep), up(ei), ne)}
        touched = postings_touched(qi.cpu().numpy().view(np.uint32), qn.cpu().numpy(), di.cpu().numpy().view(np.uint32), dn.cpu().numpy(), n_words)
        self.info = {"keyframes": D, "queries": B, "n_words": n_words, "postings_in_the_file": int(np.maximum(dn.cpu().numpy(), 0).sum()),
                     "postings_touched_per_query": stats(touched), "pairs_per_query_dense": D}

    def call(self, h, kind, out=None, stream=None):
        return h.query_device(kind, self.db, self.qs[kind], CCAP, NCAND, out=out, stream=stream.cuda_stream)

    def equal(self, h, dense, stream):
        """Both kinds on a zeroed score array: every array of the result and the OUT scores equal the dense call's."""
        import torch
        for kind in self.qs:
            got = []
            for handle in (dense, h):
                self.db.kf_score.zero_()
                torch.cuda.synchronize()
                r = self.call(handle, kind, stream=stream)
                stream.synchronize()
                got.append([None if a is None else a.cpu().numpy() for a in (r.cand, r.ncand, r.merge, r.nmerge, r.stats, self.db.kf_score)])
            for a, b in zip(*got):
                assert (a is None) == (b is None) and (a is None or np.array_equal(a.view(np.uint32), b.view(np.uint32))), (self.name, kind)
            assert got[0][1].min() >= 0
        return got[0]


def handles(n_words):
    from orb_slam3_modified_amd import placeindex as px
    hs = {}
    for g in GROUPS:
        os.environ["ORBX_PLACEINDEX_GROUP"] = str(g)
        hs[g] = px.PlaceIndex(n_words, 0)
    del os.environ["ORBX_PLACEINDEX_GROUP"]
    return hs


def measure(w, dense, stream, repeats):
    import dataclasses
    from orb_slam3_modified_amd import placeindex as px
    from tests import place_model as pm
    hs = handles(w.n_words)
    tails = {t: px.PlaceIndex(w.n_words, 0) for t in TAILS}
    for h in hs.values():
        h.sync_device(w.db, stream=stream.cuda_stream)
    for t, h in tails.items():
        h.sync_device(dataclasses.replace(w.db, count=w.D - t), stream=stream.cuda_stream)
    for h in list(hs.values()) + list(tails.values()):
        ref = w.equal(h, dense, stream)
    outs = {k: w.call(dense, k, stream=stream) for k in w.qs}
    variants = {}
    for kind, kn in ((pm.RELOC, "reloc"), (pm.NBEST, "nbest")):
        variants["d_dense_" + kn] = lambda kind=kind: w.call(dense, kind, outs[kind], stream)
        for g, h in hs.items():
            variants["i_index_%s_group_%d" % (kn, g)] = lambda kind=kind, h=h: w.call(h, kind, outs[kind], stream)
    for t, h in tails.items():
        variants["t_index_nbest_tail_%d" % t] = lambda h=h: w.call(h, pm.NBEST, outs[pm.NBEST], stream)
    variants["s_sync"] = lambda: hs[16].sync_device(w.db, stream=stream.cuda_stream)
    ms = interleaved(stream, variants, repeats)
    res = dict(w.info, rows_in_the_query_median=int(np.median(ref[4][:, 0])), scored_rows_median=int(np.median(ref[4][:, 1])), **ms)
    for kn in ("reloc", "nbest"):
        res["index_over_dense_" + kn] = {g: round(ms["i_index_%s_group_%d" % (kn, g)]["median"] / ms["d_dense_" + kn]["median"], 2) for g in GROUPS}
    for h in list(hs.values()) + list(tails.values()):
        h.close()
    return res


def worlds(B, train_frames, which):
    import torch
    if "euroc" in which:
        (qi, qv, qn), n_words, info = euroc_vectors(B, train_frames)
        for D in (2000, 4096):
            pick = torch.from_numpy((np.arange(D) % B).astype(np.int64)).to(qi.device)
            yield "euroc_D_%d" % D, World("euroc_D_%d" % D, (qi, qv, qn), (qi[pick].contiguous(), qv[pick].contiguous(), qn[pick].contiguous()), n_words), info
    if "sparse" in which:
        q, d, n_words = sparse_vectors(B, 4096, 1024)
        yield "sparse_D_4096", World("sparse_D_4096", q, d, n_words), {"scenes": B, "words_per_scene": 3000, "entries_per_vector": 1000}


def run(B, repeats, train_frames, which):
    import torch
    from orb_slam3_modified_amd import place as pl
    stream, dense, res = torch.cuda.Stream(device=torch.device("cuda:0")), pl.PlaceBatch(0), {}
    for name, w, info in worlds(B, train_frames, which):
        res[name] = dict(measure(w, dense, stream, repeats), source=info)
    dense.close()
    return res


def trace_child(B, train_frames, which, calls):
    """Under the profiler: per world a sync, three warm-up calls, a second sync (the marker: k_index_scatter) and `calls` N-best calls."""
    import torch
    from orb_slam3_modified_amd import placeindex as px
    from tests import place_model as pm
    stream = torch.cuda.Stream(device=torch.device("cuda:0"))
    for name, w, _ in worlds(B, train_frames, which):
        h = px.PlaceIndex(w.n_words, 0)
        h.sync_device(w.db, stream=stream.cuda_stream)
        out = w.call(h, pm.NBEST, stream=stream)
        for _ in range(2):
            w.call(h, pm.NBEST, out, stream)
        h.sync_device(w.db, stream=stream.cuda_stream)
        for _ in range(calls):
            w.call(h, pm.NBEST, out, stream)
        stream.synchronize()
        h.close()
        print("TRACED " + name, flush=True)


def stage_shares(rows, names, calls):
    """rows: (kernel name, start ns, end ns) in time order.  After every second k_index_scatter come `calls` indexed calls of one world."""
    marks = [i for i, r in enumerate(rows) if "k_index_scatter" in r[0]]
    out = {}
    for name, m in zip(names, marks[1::2]):
        end = next((i for i in range(m + 1, len(rows)) if "k_index_hist" in rows[i][0]), len(rows))
        sums, other = {k: 0.0 for k in STAGES}, set()
        for kn, t0, t1 in rows[m + 1:end]:
            hit = [stage for stage, keys in STAGES.items() if any(k in kn for k in keys)]
            if hit:
                sums[hit[0]] += (t1 - t0) * 1e-6 / calls
            else:
                other.add(kn[:60])
        total = sum(sums.values())
        out[name] = {"kernel_ms_per_call": {k: round(v, 4) for k, v in sums.items()}, "kernel_ms_total": round(total, 4),
                     "share": {k: round(v / total, 3) if total else None for k, v in sums.items()}, "kernels_not_counted": sorted(other)}
    return out


def trace(args, names):
    if shutil.which("rocprofv3") is None:
        return {"not_measured": "rocprofv3 not found"}
    tmp = tempfile.mkdtemp(prefix="orbx_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "-f", "csv", "-d", tmp, "-o", "trace", "--", sys.executable, os.path.abspath(__file__), "--trace-child",
               "--frames", str(args.frames), "--train-frames", str(args.train_frames), "--worlds", args.worlds, "--trace-calls", str(args.trace_calls)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.limit)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if p.returncode != 0 or not files:
            print(p.stdout[-3000:])
            return {"not_measured": "the traced run failed (exit %d)" % p.returncode}
        rows = []
        for f in files:
            for r in csv.DictReader(open(f)):
                rows.append((r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
        rows.sort(key=lambda r: r[1])
        return stage_shares(rows, names, args.trace_calls)
    except subprocess.TimeoutExpired:
        return {"not_measured": "the traced run ran into its time limit"}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--train-frames", type=int, default=1088, help="480 x 640 frames whose descriptors train the tree (1088 -> > 10^6)")
    ap.add_argument("--worlds", default="euroc,sparse")
    ap.add_argument("--trace", action="store_true", help="a second run under rocprofv3 --kernel-trace for the kernel groups' shares")
    ap.add_argument("--trace-calls", type=int, default=5)
    ap.add_argument("--limit", type=int, default=540, help="seconds each measuring child may take")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    which = args.worlds.split(",")
    if args.child:
        print("RESULT " + json.dumps(run(args.frames, args.repeats, args.train_frames, which)), flush=True)
        return 0
    if args.trace_child:
        trace_child(args.frames, args.train_frames, which, args.trace_calls)
        return 0
    from orb_slam3_modified_amd import build
    out = {"stamp": build.stamp(), "repeats": args.repeats, "clocks_before": clocks()}
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--frames", str(args.frames), "--repeats", str(args.repeats), "--train-frames",
           str(args.train_frames), "--worlds", args.worlds]
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
    out["worlds"] = json.loads(lines[-1][7:])
    out["clocks_after"] = clocks()
    if args.trace:
        out["kernel_groups_nbest_fully_synced_group_16"] = trace(args, list(out["worlds"]))
    write_result(args.out, "tools/placeindex_times.py: place recognition through the device inverted file against the dense call, interleaved "
                 "HIP-event medians [min, max] of --repeats rounds (ms); kernel groups: rocprofv3 kernel trace, a run of its own", out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
