#!/usr/bin/env python3
"""Writes tests/golden/voc_train.npz: inputs and outputs of the REFERENCE'S OWN TemplatedVocabulary::create.

Compiles tests/support/voc_train_ref.cpp together with the reference's DBoW2 sources (Thirdparty/DBoW2, over oracle/ref_shims: include path
only) into a temporary directory, runs one configuration per process (DUtils::Random::SeedRandOnce(seed), then create) and stores the node
arrays exactly (parent, leaf flag, descriptor, weight as float64).  Needs the reference tree (REFROOT, default /root/reference), so it runs
only where that is present.  Configurations the reference does not complete (it dereferences a released cv::Mat on an empty cluster) are
reported and left out.

  python tools/make_voc_train_golden.py [--large] [--check]
    --check  rebuild in memory and compare with the committed file (exit 1 on a difference)
    --large  the second file, tests/golden/voc_train_large.npz: the reference's create on the generated sets of tests/voc_train_cases.py
             (outputs, settings and the inputs' SHA-256 only; the numpy model's empty_clusters / iterations and its device / host node
             counts per threshold go under model_ keys, the reference does not report them)
time_reference() times the reference-compiled create on other descriptors (tools/voc_train_times.py uses it).
"""
from __future__ import annotations

import argparse
import os
import platform
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REFROOT = os.environ.get("REFROOT", "/root/reference")
GOLDEN = os.path.join(ROOT, "tests", "golden", "voc_train.npz")
GOLDEN_LARGE = os.path.join(ROOT, "tests", "golden", "voc_train_large.npz")
DBOW = ["DBoW2/BowVector.cpp", "DBoW2/FeatureVector.cpp", "DBoW2/ScoringObject.cpp", "DBoW2/FORB.cpp", "DUtils/Random.cpp", "DUtils/Timestamp.cpp"]

# (name, descriptor set, k, L, weighting, scoring, seed); weighting 0 TF_IDF, 1 TF, 2 IDF, 3 BINARY
CONFIGS = [
    ("nat_k10_L3_tfidf_s1", "natural", 10, 3, 0, 0, 1),
    ("nat_k10_L3_tfidf_s2", "natural", 10, 3, 0, 0, 2),
    ("nat_k16_L1_idf_s6", "natural", 16, 1, 2, 0, 6),
    ("synth_k5_L4_tf_s3", "synth", 5, 4, 1, 1, 3),
    ("synth_k2_L4_idf_s4", "synth", 2, 4, 2, 0, 4),
    ("synth_k16_L2_binary_s5", "synth", 16, 2, 3, 0, 5),
    ("synth_k10_L4_tfidf_s11", "synth", 10, 4, 0, 0, 11),
    ("clustered_k10_L3_tfidf_s7", "clustered", 10, 3, 0, 0, 7),
    ("clustered_k5_L2_tf_s8", "clustered", 5, 2, 1, 0, 8),
    ("clustered_k10_L2_idf_s21", "clustered", 10, 2, 2, 0, 21),
    ("few_k10_L2_tfidf_s9", "few", 10, 2, 0, 0, 9),
    ("few_k5_L3_idf_s10", "few", 5, 3, 2, 0, 10),
    ("tiny_k10_L2_tfidf_s12", "tiny", 10, 2, 0, 0, 12),
]


def descriptor_sets() -> dict:
    """name -> (desc (N, 32) uint8, doc offsets (ndocs + 1) int64)."""
    from oracle import pyoracle as po
    from orb_slam3_modified_amd import synth
    sets = {}
    z = np.load(os.path.join(ROOT, "tests", "golden", "natural_crops.npz"))
    docs = [z["result_640x480_desc"], z["pineapple_640x480_desc"], z["teaser_752x480_desc"]]   # the reference extractor's descriptors
    sets["natural"] = docs
    ex = po.OracleExtractor(500, 1.2, 6, 20, 7)
    sets["synth"] = [ex.extract(img, (0, 1000))[1] for img in synth.make_stream(6, 240, 320, 4242)]
    rng = np.random.default_rng(97)
    centres = rng.integers(0, 256, (60, 32), dtype=np.uint8)
    pick = rng.integers(0, 60, 3000)
    flips = rng.random((3000, 256)) < 0.03          # near-duplicates around 60 centres
    clustered = np.packbits(np.unpackbits(centres[pick], axis=1) ^ flips, axis=1)
    sets["clustered"] = [clustered[i:i + 100] for i in range(0, 3000, 100)]
    distinct = rng.integers(0, 256, (4, 32), dtype=np.uint8)   # fewer distinct descriptors than k: the seeding stops early
    sets["few"] = [distinct[rng.integers(0, 4, 40)] for _ in range(3)]
    sets["tiny"] = [rng.integers(0, 256, (4, 32), dtype=np.uint8), rng.integers(0, 256, (3, 32), dtype=np.uint8)]
    out = {}
    for name, docs in sets.items():
        docs = [np.ascontiguousarray(d, np.uint8).reshape(-1, 32) for d in docs]
        off = np.zeros(len(docs) + 1, np.int64)
        off[1:] = np.cumsum([len(d) for d in docs])
        out[name] = (np.concatenate(docs), off)
    return out


def build_driver(tmp: str) -> str:
    ref = os.path.join(REFROOT, "Thirdparty", "DBoW2")
    exe = os.path.join(tmp, "voc_train_ref")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-w", "-I" + os.path.join(ROOT, "oracle", "ref_shims"), "-I" + ref,
                           os.path.join(ROOT, "tests", "support", "voc_train_ref.cpp")] + [os.path.join(ref, s) for s in DBOW] + ["-o", exe])
    return exe


def run_reference(exe: str, tmp: str, desc, off, k, L, w, s, seed):
    """-> ((parent, leaf, desc, weight), seconds) or (None, returncode) when the reference did not complete."""
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([k, L, w, s], np.int32).tobytes() + np.array([seed], np.uint32).tobytes() + np.array([len(off) - 1], np.int32).tobytes())
        f.write(np.asarray(off, np.int64).tobytes() + np.ascontiguousarray(desc, np.uint8).tobytes())
    t0 = time.perf_counter()
    p = subprocess.run([exe, fin, fout], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    dt = time.perf_counter() - t0
    if p.returncode != 0:
        return None, p.returncode
    b = open(fout, "rb").read()
    n = int(np.frombuffer(b, np.int64, 1)[0])
    o = 8
    parent = np.frombuffer(b, np.int32, n, o); o += 4 * n
    leaf = np.frombuffer(b, np.uint8, n, o); o += n
    d = np.frombuffer(b, np.uint8, 32 * n, o).reshape(n, 32); o += 32 * n
    weight = np.frombuffer(b, np.float64, n, o)
    return (parent.copy(), leaf.copy(), d.copy(), weight.copy()), dt


def make() -> dict:
    sets = descriptor_sets()
    tmp = tempfile.mkdtemp(prefix="voc_train_ref_")
    try:
        exe = build_driver(tmp)
        out = {}
        for name, (desc, off) in sets.items():
            out[f"in_{name}_desc"], out[f"in_{name}_off"] = desc, off
        names, crashed = [], []
        for name, dset, k, L, w, s, seed in CONFIGS:
            desc, off = sets[dset]
            res, info = run_reference(exe, tmp, desc, off, k, L, w, s, seed)
            if res is None:
                crashed.append((name, info))
                continue
            names.append(name)
            out[f"cfg_{name}"] = np.array([k, L, w, s, seed], np.int64)
            out[f"cfg_{name}_set"] = np.array(dset)
            for key, a in zip(("parent", "leaf", "desc", "weight"), res):
                out[f"out_{name}_{key}"] = a
        out["configs"] = np.array(names)
        for name, rc in crashed:
            print(f"reference create did not complete on {name} (exit {rc}): left out", file=sys.stderr)
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def make_large() -> dict:
    """Every case of tests/voc_train_cases.py through the reference; a case it does not complete is an error (take another seed)."""
    from tests import voc_train_cases as VC, voc_train_model as M
    tmp = tempfile.mkdtemp(prefix="voc_train_ref_")
    try:
        exe = build_driver(tmp)
        out = {"cases": np.array(list(VC.CASES))}
        for name, c in VC.CASES.items():
            desc, off = VC.generate(name)
            res, info = run_reference(exe, tmp, desc, off, c["k"], c["L"], c["weighting"], c["scoring"], c["seed"])
            if res is None:
                raise SystemExit(f"reference create did not complete on {name} (exit {info}): take another seed")
            trace = []
            _, st = M.create(desc, off, c["k"], c["L"], c["weighting"], c["seed"], trace=trace)
            out[f"cfg_{name}"] = np.array([c["k"], c["L"], c["weighting"], c["scoring"], c["seed"], c["mid"]], np.int64)
            out[f"gen_{name}"] = np.array(c["gen"])
            out[f"args_{name}"] = np.array(c["args"], np.float64)
            out[f"off_{name}"] = off
            out[f"sha_{name}"] = np.array(VC.digest(desc, off))
            for key, a in zip(("parent", "leaf", "desc", "weight"), res):
                out[f"out_{name}_{key}"] = a
            out[f"model_{name}_stats"] = np.array([st["empty_clusters"], st["iterations"]], np.int64)
            out[f"model_{name}_split"] = np.array([(thr,) + VC.split(trace, c["k"], thr)
                                                   for thr in (c["k"] + 1, c["mid"], VC.DEFAULT_MIN_NODE, VC.HOST_ONLY)], np.int64)
            print(f"{name}: {len(desc)} descriptors, {len(res[0])} nodes, reference {info:.1f} s", file=sys.stderr)
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def time_reference(desc, off, k, L, w=0, s=0, seed=1):
    """(wall seconds, node arrays) of the reference-compiled create (one core) on the given descriptors."""
    tmp = tempfile.mkdtemp(prefix="voc_train_ref_")
    try:
        exe = build_driver(tmp)
        res, dt = run_reference(exe, tmp, desc, off, k, L, w, s, seed)
        if res is None:
            raise RuntimeError(f"reference create did not complete (exit {dt})")
        return dt, res
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def cpu_name() -> str:
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--large", action="store_true")
    a = ap.parse_args()
    out = make_large() if a.large else make()
    golden, pin = (GOLDEN_LARGE, "LARGE_SHA256") if a.large else (GOLDEN, "GOLDEN_SHA256")
    if a.check:
        z = np.load(golden)
        same = sorted(z.files) == sorted(out) and all(np.array_equal(z[f], out[f]) for f in z.files)
        print("golden reproduced bit for bit" if same else "golden DIFFERS")
        sys.exit(0 if same else 1)
    np.savez_compressed(golden, **out)
    import hashlib
    sha = hashlib.sha256(open(golden, "rb").read()).hexdigest()
    print(f"wrote {golden}: {len(out['cases' if a.large else 'configs'])} configurations, {os.path.getsize(golden)} bytes, sha256 {sha}"
          f" (tests/test_voc_train_model.py: {pin})")


if __name__ == "__main__":
    main()
