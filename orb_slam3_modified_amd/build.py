"""In-tree build of the project's shared libraries.  HIP, gfx950 only.  `python -m orb_slam3_modified_amd.build [--force]`.

LIBS is the one place that knows them, one record per library; what is stale, what is compiled and what is linked all follow from it:
  liborbx.so         the product (include/orbx.h): the top level of csrc/, which kernels_hash() stamps
  liborbx_debug.so   the diagnostic ABI (include/orbx_debug.h): stage dumps and numeric test hooks for the parity tests and the profiling
                     tools; the product library has none of them
  liborbx_train.so   vocabulary training (include/orbx_train.h)
  liborbx_stereo.so  the batched stereo front-end (include/orbx_stereo.h)
  liborbx_bow.so     the batched bag of words (include/orbx_bow.h)
  liborbx_match.so   the batched SearchByBoW (include/orbx_match.h)
  liborbx_initmatch.so  the batched SearchForInitialization (include/orbx_initmatch.h)
  liborbx_trimatch.so   the batched SearchForTriangulation (include/orbx_trimatch.h)
  liborbx_fuse.so       the batched Fuse search (include/orbx_fuse.h)
  liborbx_mpdesc.so     the batched ComputeDistinctiveDescriptors (include/orbx_mpdesc.h)
  liborbx_score.so      the six DBoW2 scorings for two batches of BowVectors (include/orbx_score.h); takes nothing from the product
  liborbx_fisheye.so    the batched two-camera rig front-end (include/orbx_fisheye.h)
  liborbx_localmatch.so the batched SearchLocalPoints (include/orbx_localmatch.h)
  liborbx_lastmatch.so  the batched SearchByProjection(Frame, LastFrame) (include/orbx_lastmatch.h)
  liborbx_projmatch.so  the batched relocalization and Sim3 SearchByProjection (include/orbx_projmatch.h)
  liborbx_place.so      the batched place recognition: relocalization and N-best candidates (include/orbx_place.h); takes nothing from
                        the product
  liborbx_placeindex.so the same candidates through a device inverted file that grows (include/orbx_placeindex.h); takes nothing from it
  liborbx_frustum.so    the batched Frame::isInFrustum + PredictScale, written as liborbx_localmatch.so's point rows (include/orbx_frustum.h);
                        takes nothing from the product
  liborbx_project.so    the Sophus Tcw * x projection fronts of the LastFrame, relocalization and Fuse matchers, written as those
                        matchers' rows (include/orbx_project.h); takes nothing from the product
  liborbx_sim3.so       the projection fronts of LoopClosing's Sim3 callers and SearchBySim3's agreement pass (include/orbx_sim3.h);
                        takes nothing from the product
  liborbx_rigmatch.so   the two-camera rig blocks of SearchLocalPoints and SearchByProjection(Frame, LastFrame), batched
                        (include/orbx_rigmatch.h)
  liborbx_rigbow.so     the two-camera rig block of SearchByBoW, batched, and the stacked rig frame it runs on (include/orbx_rigbow.h);
                        takes nothing from the product
  liborbx_mpgeom.so     the batched MapPoint::UpdateNormalAndDepth, written in place into the projection fronts' table of map points
                        (include/orbx_mpgeom.h); takes nothing from the product
The libraries beside the product link liborbx.so and use its ABI (and orbx_internal.h where they read a context's buffers).  Their sources sit
in subdirectories of csrc/, outside kernels_hash(): the committed counter files measure the product's kernels, which they do not change.
A new one is one more record ("Adding a side library")."""
from __future__ import annotations

import os
import subprocess
import sys
from typing import NamedTuple

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.environ.get("ORBX_BUILD_OUT") or os.path.join(HERE, "liborbx.so")   # ORBX_BUILD_OUT (+ ORBX_EXTRA_FLAGS): experiment builds beside the product
SOURCES = ["orbx_extractor.hip", "orbx_matcher.hip", "orbx_search.hip", "orbx_window.hip", "orbx_kfdb.hip", "orbx_replay.hip"]
DEBUG_OUT = os.path.join(os.path.dirname(OUT), "liborbx_debug.so")
DEBUG_SOURCE = "orbx_debug.hip"     # = the extractor's translation unit with ORBX_DEBUG_ABI
TRAIN_OUT = os.path.join(os.path.dirname(OUT), "liborbx_train.so")
TRAIN_SOURCE = os.path.join("train", "orbx_train.hip")
STEREO_OUT = os.path.join(os.path.dirname(OUT), "liborbx_stereo.so")
STEREO_SOURCE = os.path.join("stereo", "orbx_stereo.hip")
BOW_OUT = os.path.join(os.path.dirname(OUT), "liborbx_bow.so")
BOW_SOURCE = os.path.join("bow", "orbx_bow.hip")
MATCH_OUT = os.path.join(os.path.dirname(OUT), "liborbx_match.so")
MATCH_SOURCE = os.path.join("match", "orbx_match.hip")
INITMATCH_OUT = os.path.join(os.path.dirname(OUT), "liborbx_initmatch.so")
INITMATCH_SOURCE = os.path.join("initmatch", "orbx_initmatch.hip")
TRIMATCH_OUT = os.path.join(os.path.dirname(OUT), "liborbx_trimatch.so")
TRIMATCH_SOURCE = os.path.join("trimatch", "orbx_trimatch.hip")
FUSE_OUT = os.path.join(os.path.dirname(OUT), "liborbx_fuse.so")
FUSE_SOURCE = os.path.join("fuse", "orbx_fuse.hip")
MPDESC_OUT = os.path.join(os.path.dirname(OUT), "liborbx_mpdesc.so")
MPDESC_SOURCE = os.path.join("mpdesc", "orbx_mpdesc.hip")
SCORE_OUT = os.path.join(os.path.dirname(OUT), "liborbx_score.so")
SCORE_SOURCE = os.path.join("score", "orbx_score.hip")
FISHEYE_OUT = os.path.join(os.path.dirname(OUT), "liborbx_fisheye.so")
FISHEYE_SOURCE = os.path.join("fisheye", "orbx_fisheye.hip")
LOCALMATCH_OUT = os.path.join(os.path.dirname(OUT), "liborbx_localmatch.so")
LOCALMATCH_SOURCE = os.path.join("localmatch", "orbx_localmatch.hip")
LASTMATCH_OUT = os.path.join(os.path.dirname(OUT), "liborbx_lastmatch.so")
LASTMATCH_SOURCE = os.path.join("lastmatch", "orbx_lastmatch.hip")
PROJMATCH_OUT = os.path.join(os.path.dirname(OUT), "liborbx_projmatch.so")
PROJMATCH_SOURCE = os.path.join("projmatch", "orbx_projmatch.hip")
WINDOW_CORE = (os.path.join("side", "orbx_window_device.h"), os.path.join("side", "orbx_window_host.h"))   # what those three and the rig matcher share
PLACE_OUT = os.path.join(os.path.dirname(OUT), "liborbx_place.so")
PLACE_SOURCE = os.path.join("place", "orbx_place.hip")
PLACE_KERNELS = os.path.join("place", "orbx_place_kernels.h")   # what the two place libraries share
PLACEINDEX_OUT = os.path.join(os.path.dirname(OUT), "liborbx_placeindex.so")
PLACEINDEX_SOURCE = os.path.join("placeindex", "orbx_placeindex.hip")
FRUSTUM_OUT = os.path.join(os.path.dirname(OUT), "liborbx_frustum.so")
FRUSTUM_SOURCE = os.path.join("frustum", "orbx_frustum.hip")
PROJECT_OUT = os.path.join(os.path.dirname(OUT), "liborbx_project.so")
PROJECT_SOURCE = os.path.join("project", "orbx_project.hip")
SIM3_OUT = os.path.join(os.path.dirname(OUT), "liborbx_sim3.so")
SIM3_SOURCE = os.path.join("sim3", "orbx_sim3.hip")
RIGMATCH_OUT = os.path.join(os.path.dirname(OUT), "liborbx_rigmatch.so")
RIGMATCH_SOURCE = os.path.join("rigmatch", "orbx_rigmatch.hip")
RIGBOW_OUT = os.path.join(os.path.dirname(OUT), "liborbx_rigbow.so")
RIGBOW_SOURCE = os.path.join("rigbow", "orbx_rigbow.hip")
MPGEOM_OUT = os.path.join(os.path.dirname(OUT), "liborbx_mpgeom.so")
MPGEOM_SOURCE = os.path.join("mpgeom", "orbx_mpgeom.hip")
FRONT_CORE = (os.path.join("side", "orbx_front_device.h"), os.path.join("side", "orbx_front_host.h"))   # what the three projection fronts share
PAIR_CORE = (os.path.join("side", "orbx_pair_device.h"), os.path.join("side", "orbx_pair_host.h"))   # what the four pair matchers share


class Lib(NamedTuple):
    out: str
    sources: tuple          # relative to csrc/, one object each
    hidden: bool = False    # -fvisibility=hidden: the library exports its extern "C" entry points alone
    product: bool = False   # links liborbx.so: what it takes from the product it takes at load time ($ORIGIN)
    deps: tuple = ()        # further files of csrc/ its objects are made from


LIBS = (Lib(OUT, tuple(SOURCES)),
        Lib(DEBUG_OUT, (DEBUG_SOURCE,), hidden=True, product=True, deps=("orbx_extractor.hip",)),   # it IS the extractor's translation unit
        Lib(TRAIN_OUT, (TRAIN_SOURCE,), product=True),
        Lib(STEREO_OUT, (STEREO_SOURCE,), hidden=True, product=True),
        Lib(BOW_OUT, (BOW_SOURCE,), hidden=True, product=True),
        Lib(MATCH_OUT, (MATCH_SOURCE,), hidden=True, product=True, deps=PAIR_CORE),
        Lib(INITMATCH_OUT, (INITMATCH_SOURCE,), hidden=True, product=True, deps=PAIR_CORE),
        Lib(TRIMATCH_OUT, (TRIMATCH_SOURCE,), hidden=True, product=True, deps=PAIR_CORE),
        Lib(FUSE_OUT, (FUSE_SOURCE,), hidden=True, product=True),
        Lib(MPDESC_OUT, (MPDESC_SOURCE,), hidden=True, product=True),
        Lib(SCORE_OUT, (SCORE_SOURCE,), hidden=True),
        Lib(FISHEYE_OUT, (FISHEYE_SOURCE,), hidden=True, product=True),
        Lib(LOCALMATCH_OUT, (LOCALMATCH_SOURCE,), hidden=True, product=True, deps=WINDOW_CORE),
        Lib(LASTMATCH_OUT, (LASTMATCH_SOURCE,), hidden=True, product=True, deps=WINDOW_CORE),
        Lib(PROJMATCH_OUT, (PROJMATCH_SOURCE,), hidden=True, product=True, deps=WINDOW_CORE),
        Lib(PLACE_OUT, (PLACE_SOURCE,), hidden=True, deps=(PLACE_KERNELS,)),
        Lib(PLACEINDEX_OUT, (PLACEINDEX_SOURCE,), hidden=True, deps=(PLACE_KERNELS,)),
        Lib(FRUSTUM_OUT, (FRUSTUM_SOURCE,), hidden=True, deps=FRONT_CORE),
        Lib(PROJECT_OUT, (PROJECT_SOURCE,), hidden=True, deps=FRONT_CORE),
        Lib(SIM3_OUT, (SIM3_SOURCE,), hidden=True, deps=FRONT_CORE),
        Lib(RIGMATCH_OUT, (RIGMATCH_SOURCE,), hidden=True, deps=WINDOW_CORE),
        Lib(RIGBOW_OUT, (RIGBOW_SOURCE,), hidden=True, deps=PAIR_CORE),
        Lib(MPGEOM_OUT, (MPGEOM_SOURCE,), hidden=True, deps=(os.path.join("side", "orbx_handle.h"), os.path.join("side", "orbx_front_device.h"))))
HEADERS = ("orbx.h", "orbx_debug.h", "orbx_train.h", "orbx_stereo.h", "orbx_bow.h", "orbx_match.h", "orbx_initmatch.h", "orbx_trimatch.h",
           "orbx_fuse.h", "orbx_mpdesc.h", "orbx_score.h", "orbx_fisheye.h", "orbx_localmatch.h", "orbx_lastmatch.h",
           "orbx_projmatch.h", "orbx_place.h", "orbx_placeindex.h", "orbx_frustum.h", "orbx_project.h", "orbx_sim3.h", "orbx_rigmatch.h",
           "orbx_rigbow.h", "orbx_mpgeom.h")
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


def _headers(below: bool) -> list:
    """What an object may include: include/, the headers of csrc/'s top level and, for a source in a subdirectory of csrc/, those of every
    subdirectory too (csrc/side/)."""
    hs = [os.path.join(HERE, "..", "include", h) for h in HEADERS]
    for d, _, files in os.walk(CSRC):
        if below or d == CSRC:
            hs += [os.path.join(d, f) for f in files if f.endswith((".h", ".inc")) or f == "orbx_kernels.hip"]
    return hs


def _stale() -> bool:
    if not all(os.path.exists(lib.out) for lib in LIBS):
        return True
    t = min(os.path.getmtime(lib.out) for lib in LIBS)
    deps = _headers(True) + [os.path.join(CSRC, f) for lib in LIBS for f in lib.sources + lib.deps]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = True) -> str:
    """One object per source (compiled in parallel, rebuilt only when the source or a header is newer), then one link per library."""
    if not (force or _stale()):
        return OUT
    from concurrent.futures import ThreadPoolExecutor
    hipcc = os.environ.get("HIPCC", "hipcc")
    extra = os.environ.get("ORBX_EXTRA_FLAGS", "").split()
    objdir = os.path.join(HERE, "build") if OUT == os.path.join(HERE, "liborbx.so") else OUT + ".obj"   # an experiment build keeps its objects beside it
    os.makedirs(objdir, exist_ok=True)
    cflags = [f for f in FLAGS if f not in ("-shared", "-ldl")] + extra
    tag = os.path.join(objdir, ".flags")
    flags_now = " ".join([hipcc] + cflags)
    same_flags = os.path.exists(tag) and open(tag).read() == flags_now

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=CSRC)

    def compile_one(job):
        lib, src = job
        obj = os.path.join(objdir, os.path.basename(src).replace(".hip", ".o"))
        made_from = [os.path.join(CSRC, f) for f in (src,) + lib.deps] + _headers(os.path.dirname(src) != "")
        if force or not same_flags or not os.path.exists(obj) or os.path.getmtime(obj) <= max(os.path.getmtime(f) for f in made_from):
            run([hipcc] + cflags + (["-fvisibility=hidden"] if lib.hidden else []) + ["-c", os.path.join(CSRC, src), "-o", obj])
        return obj

    jobs = [(lib, src) for lib in LIBS for src in lib.sources]
    with ThreadPoolExecutor(max_workers=len(SOURCES) + 1) as ex:
        objs = dict(zip(jobs, ex.map(compile_one, jobs)))
    open(tag, "w").write(flags_now)
    against_product = ["-L", os.path.dirname(OUT), "-l:" + os.path.basename(OUT), "-Wl,-rpath,$ORIGIN"]
    for lib in LIBS:
        run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib.out] + [objs[lib, src] for src in lib.sources] +
            (against_product if lib.product else []) + ["-ldl"])
    return OUT


if __name__ == "__main__":
    build(force="--force" in sys.argv)
