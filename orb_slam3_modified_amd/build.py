"""In-tree build of liborbx.so — the product —, of liborbx_train.so — vocabulary training (include/orbx_train.h) —, of liborbx_stereo.so — the
batched stereo front-end (include/orbx_stereo.h) —, of liborbx_bow.so — the batched bag of words (include/orbx_bow.h) — and of liborbx_debug.so — the diagnostic ABI (include/orbx_debug.h: stage dumps and numeric test
hooks for the parity tests and the profiling tools; the product library has none of them).  HIP, gfx950 only.
`python -m orb_slam3_modified_amd.build [--force]`."""
from __future__ import annotations

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.environ.get("ORBX_BUILD_OUT") or os.path.join(HERE, "liborbx.so")   # ORBX_BUILD_OUT (+ ORBX_EXTRA_FLAGS): experiment builds beside the product
SOURCES = ["orbx_extractor.hip", "orbx_matcher.hip", "orbx_search.hip", "orbx_window.hip", "orbx_kfdb.hip", "orbx_replay.hip"]
DEBUG_OUT = os.path.join(os.path.dirname(OUT), "liborbx_debug.so")
DEBUG_SOURCE = "orbx_debug.hip"     # = the extractor's translation unit with ORBX_DEBUG_ABI; -fvisibility=hidden: exports orbx_debug_* alone
# liborbx_train.so — vocabulary training (include/orbx_train.h): offline work beside the product, links liborbx.so and uses only its ABI.  Its
# source sits in csrc/train/, outside kernels_hash(): the committed counter files measure the product's kernels, which it does not change.
TRAIN_OUT = os.path.join(os.path.dirname(OUT), "liborbx_train.so")
TRAIN_SOURCE = os.path.join("train", "orbx_train.hip")
# liborbx_stereo.so — the batched stereo front-end (include/orbx_stereo.h): links liborbx.so for the product calls it makes and reads the buffers a
# product context left behind (orbx_internal.h), like the debug library; -fvisibility=hidden: exports orbx_stereo_* alone.  Source in csrc/stereo/,
# outside kernels_hash() for the same reason as the training library's.
STEREO_OUT = os.path.join(os.path.dirname(OUT), "liborbx_stereo.so")
STEREO_SOURCE = os.path.join("stereo", "orbx_stereo.hip")
# liborbx_bow.so — the batched bag of words (include/orbx_bow.h): BowVectors, FeatureVectors and L1 score matrices for B frames.  Built exactly like
# the stereo library: links liborbx.so, -fvisibility=hidden (exports orbx_bow_* alone), source in csrc/bow/, outside kernels_hash().
BOW_OUT = os.path.join(os.path.dirname(OUT), "liborbx_bow.so")
BOW_SOURCE = os.path.join("bow", "orbx_bow.hip")
HEADERS = ("orbx.h", "orbx_debug.h", "orbx_train.h", "orbx_stereo.h", "orbx_bow.h")
# -ffp-contract=off: the float paths (fastAtan2 polynomial, BRIEF rotation) must not be fused into FMAs,
# the CPU reference evaluates them as separate IEEE operations (DESIGN.md "bit-exactness").
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall",
         "-Wno-unused-function", "-ldl"]


def kernels_hash() -> str:
    """sha256 over the kernel sources (csrc/*.hip, *.h, *.inc, sorted by name), first 16 hex digits: what the committed counter files
    (profiles/pmc_*.json) are stamped with, so that bench.py can tell whether they were measured on THIS code."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".h", ".inc")):
            h.update(f.encode() + b"\0" + open(os.path.join(CSRC, f), "rb").read())
    return h.hexdigest()[:16]


def stamp() -> dict:
    """{kernels_hash, commit, date} for evidence files: the commit comes from ORBX_COMMIT (the GPU box has no .git) or `git rev-parse`."""
    import datetime
    commit = os.environ.get("ORBX_COMMIT")
    if not commit:
        try:
            commit = subprocess.check_output(["git", "-C", HERE, "rev-parse", "--short=12", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:   # noqa: BLE001
            commit = "unknown"
    return {"kernels_hash": kernels_hash(), "commit": commit, "date": datetime.datetime.utcnow().strftime("%Y-%m-%dT%H:%MZ")}


def _stale() -> bool:
    outs = (OUT, DEBUG_OUT, TRAIN_OUT, STEREO_OUT, BOW_OUT)
    if not all(os.path.exists(o) for o in outs):
        return True
    t = min(os.path.getmtime(o) for o in outs)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(CSRC, TRAIN_SOURCE), os.path.join(CSRC, STEREO_SOURCE), os.path.join(CSRC, BOW_SOURCE)] + \
           [os.path.join(HERE, "..", "include", h) for h in HEADERS]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = True) -> str:
    """One object per source (compiled in parallel, rebuilt only when the source or a header is newer), then one link."""
    if not (force or _stale()):
        return OUT
    from concurrent.futures import ThreadPoolExecutor
    hipcc = os.environ.get("HIPCC", "hipcc")
    extra = os.environ.get("ORBX_EXTRA_FLAGS", "").split()
    objdir = os.path.join(HERE, "build") if OUT.endswith("/liborbx.so") else OUT + ".obj"
    os.makedirs(objdir, exist_ok=True)
    cflags = [f for f in FLAGS if f not in ("-shared", "-ldl")] + extra
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if not f.endswith(".hip") or f == "orbx_kernels.hip"] + \
              [os.path.join(HERE, "..", "include", h) for h in HEADERS]
    hnew = max(os.path.getmtime(h) for h in headers if os.path.isfile(h))
    tag = os.path.join(objdir, ".flags")
    flags_now = " ".join([hipcc] + cflags)
    same_flags = os.path.exists(tag) and open(tag).read() == flags_now

    def compile_one(src):
        obj = os.path.join(objdir, os.path.basename(src).replace(".hip", ".o"))
        sp = os.path.join(CSRC, src)
        newest = max(os.path.getmtime(sp), hnew)
        if src == DEBUG_SOURCE:   # it IS the extractor's translation unit
            newest = max(newest, os.path.getmtime(os.path.join(CSRC, "orbx_extractor.hip")))
        if not force and same_flags and os.path.exists(obj) and os.path.getmtime(obj) > newest:
            return obj
        cmd = [hipcc] + cflags + (["-fvisibility=hidden"] if src in (DEBUG_SOURCE, STEREO_SOURCE, BOW_SOURCE) else []) + ["-c", sp, "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=CSRC)
        return obj

    with ThreadPoolExecutor(max_workers=len(SOURCES) + 1) as ex:
        objs = list(ex.map(compile_one, SOURCES + [DEBUG_SOURCE, TRAIN_SOURCE, STEREO_SOURCE, BOW_SOURCE]))
    open(tag, "w").write(flags_now)
    # the debug library is the extractor's translation unit alone: what that unit takes from the others (the vocabulary's device view, ...) it takes
    # from liborbx.so at load time ($ORIGIN)
    # (so do the training, the stereo and the bag-of-words library)
    against_product = ["-L", os.path.dirname(OUT), "-l:" + os.path.basename(OUT), "-Wl,-rpath,$ORIGIN"]
    for out, oo, more in ((OUT, objs[:-4], []), (DEBUG_OUT, objs[-4:-3], against_product), (TRAIN_OUT, objs[-3:-2], against_product),
                          (STEREO_OUT, objs[-2:-1], against_product), (BOW_OUT, objs[-1:], against_product)):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + oo + more + ["-ldl"]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=CSRC)
    return OUT


if __name__ == "__main__":
    build(force="--force" in sys.argv)
