"""include/orbx_score.h <-> liborbx_score.so: the six DBoW2 scorings are a library of their own beside the product (CPU-only checks)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from tests import abi_util
from tests.abi_util import declared as _declared, exported as _exported

ROOT = abi_util.ROOT
KERNELS_HASH = "cfa5f580d25d496f"   # the product's kernel sources: this library changes none of them
HEADER = "orbx_score.h"
NAMES = ("create", "destroy", "last_error", "pair", "matrix_device", "matrix")


def test_build_produces_the_score_library():
    from orb_slam3_modified_amd import _lib, build
    build.build()
    assert os.path.isfile(build.SCORE_OUT) and build.SCORE_OUT == _lib.SCORE_LIB_PATH
    assert os.path.dirname(build.SCORE_OUT) == os.path.dirname(_lib.LIB_PATH) == os.path.join(ROOT, "orb_slam3_modified_amd")
    assert os.path.basename(build.SCORE_OUT) == "liborbx_score.so"
    assert HEADER in build.HEADERS
    rec = [l for l in build.LIBS if l.out == build.SCORE_OUT]
    assert len(rec) == 1 and rec[0].sources == (build.SCORE_SOURCE,) and rec[0].hidden
    assert "-ffp-contract=off" in build.FLAGS


def test_score_library_exports_exactly_its_header():
    from orb_slam3_modified_amd import _lib, build
    build.build()
    names = _declared(HEADER)
    assert names == sorted("orbx_score_" + n for n in NAMES), names
    exported = _exported(_lib.SCORE_LIB_PATH)
    assert {e for e in exported if e.startswith("orbx_")} == set(names)
    assert not [e for e in exported if not e.startswith("orbx_score_") and not e.startswith("_")], sorted(exported)[:10]   # -fvisibility=hidden


def test_the_other_libraries_keep_their_abi_and_their_kernels():
    from orb_slam3_modified_amd import _lib, build
    build.build()
    names = set(_declared(HEADER))
    for other in (_lib.LIB_PATH, _lib.BOW_LIB_PATH, _lib.MPDESC_LIB_PATH, _lib.FUSE_LIB_PATH, _lib.TRIMATCH_LIB_PATH, _lib.MATCH_LIB_PATH,
                  _lib.INITMATCH_LIB_PATH, _lib.STEREO_LIB_PATH):
        assert not names & _exported(other), other
    assert not names & set(_declared("orbx.h")) and not names & set(_declared("orbx_bow.h"))
    assert len(_declared("orbx.h")) == 100 and len(_declared("orbx_bow.h")) == 7
    assert build.kernels_hash() == KERNELS_HASH
    assert os.path.dirname(build.SCORE_SOURCE) == "score" and "orbx_score.hip" not in os.listdir(build.CSRC)
    src = open(os.path.join(build.CSRC, build.SCORE_SOURCE)).read()
    assert "side/orbx_handle.h" in src and "orbx_internal.h" not in src and "asm" not in re.sub(r"//.*", "", src)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not installed")
def test_the_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "orbx_score.h"\n'
                   "typedef char the_values[ORBX_SCORE_L1_NORM == 0 && ORBX_SCORE_L2_NORM == 1 && ORBX_SCORE_CHI_SQUARE == 2 && ORBX_SCORE_KL == 3 &&"
                   " ORBX_SCORE_BHATTACHARYYA == 4 && ORBX_SCORE_DOT_PRODUCT == 5 ? 1 : -1];\n"
                   "int main(void) { return 0; }\n")
    obj = tmp_path / "use.o"
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(obj)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-2000:]


def test_python_binding_covers_the_header():
    import orb_slam3_modified_amd
    from orb_slam3_modified_amd import _lib, build, score
    build.build()
    S = _lib.score_lib()
    assert set(S._orbx_score_symbols) == set(_declared(HEADER))
    assert orb_slam3_modified_amd.ScoreBatch is score.ScoreBatch and issubclass(score.ScoreBatch, _lib.SideHandle)
    for m in ("pair", "matrix", "matrix_device", "close"):
        assert callable(getattr(score.ScoreBatch, m))
    assert score.SCORINGS == tuple(range(6)) and score.DEVICE_SCORINGS == (0, 1, 2, 4, 5) and score.KL == 3
    src = open(os.path.join(build.CSRC, build.SCORE_SOURCE)).read()
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    for line in ("kScoreLds = %d;" % score.QUERY_LDS, "kTile = %d;" % score.DB_PER_WORKGROUP, "lds_limit = kScoreLds;",
                 'env_int("ORBX_SCORE_LDS", 0, kScoreLds, kScoreLds)'):
        assert line in src, line
    for word in ("ORBX_SCORE_LDS (0 .. %d)" % score.QUERY_LDS, "KL is host only", "glibc's double log", "LOG_EPS", "run-time log(DBL_EPSILON)",
                 "-0.0", "payload"):
        assert word in text, word


def test_the_adapter_has_score_as_and_keeps_score():
    text = open(os.path.join(ROOT, "include", "ORBVocabulary.h")).read()
    assert '#include "orbx_score.h"' in text and "double scoreAs(const DBoW2::BowVector& a, const DBoW2::BowVector& b, int scoring) const" in text
    assert "orbx_score_pair(scoring," in text
    assert "return orbx_bow_score_l1(ia.data(), va.data(), (int)ia.size(), ib.data(), vb.data(), (int)ib.size());" in text      # score(a, b) as it was


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_only_a_caller_of_score_as_needs_the_library(tmp_path):
    """A translation unit that includes the adapter and does not call scoreAs refers to no orbx_score_ name; one that calls it does."""
    refs = {}
    for tag, body in (("plain", "return v.empty() ? 0 : 1;"),
                      ("scored", "DBoW2::BowVector a, b; a.addWeight(3, 1.0); b.addWeight(3, 1.0); return v.scoreAs(a, b, 1) == 1.0 ? 0 : 1;")):
        tu = tmp_path / (tag + ".cpp")
        tu.write_text('#define ORBX_OWN_DBOW2_TYPES\n#include "ORBVocabulary.h"\nint main() { ORB_SLAM3::ORBVocabulary v; ' + body + " }\n")
        obj = tmp_path / (tag + ".o")
        p = subprocess.run(["g++", "-std=c++14", "-O1", "-I", os.path.join(ROOT, "include"), "-c", str(tu), "-o", str(obj)], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        assert p.returncode == 0, p.stdout[-3000:]
        refs[tag] = {l.split()[-1] for l in subprocess.check_output(["nm", "-u", str(obj)]).decode().splitlines()}
    assert not [n for n in refs["plain"] if n.startswith("orbx_score_")]
    assert "orbx_score_pair" in refs["scored"]


def test_bad_arguments_are_rejected_without_a_device():
    """Argument checks that come before any device call."""
    from orb_slam3_modified_amd import _lib
    S = _lib.score_lib()
    h = C.c_void_p(0)
    assert S.orbx_score_create(None, 0) == _lib.ORBX_E_INVALID
    assert b"null" in S.orbx_score_last_error(None)
    assert S.orbx_score_create(C.byref(h), -1) == _lib.ORBX_E_INVALID and not h.value
    assert b"device" in S.orbx_score_last_error(None)
    assert S.orbx_score_matrix_device(None, 0, None, None, None, 1, 1, None, None, None, 1, 1, None, None) == _lib.ORBX_E_INVALID
    assert S.orbx_score_matrix(None, 0, None, None, None, 1, None, None, None, 1, None) == _lib.ORBX_E_INVALID
    S.orbx_score_destroy(None)


@abi_util.needs_hipcc
def test_score_kernels_compile_without_scratch_one_per_scoring():
    from orb_slam3_modified_amd.build import SCORE_SOURCE
    scratch = abi_util.kernel_scratch(SCORE_SOURCE, hidden=True)
    assert sorted(re.search(r"k_scoreILi(\d)E", n).group(1) for n in scratch) == ["0", "1", "2", "4", "5"], sorted(scratch)     # no KL kernel
    assert all(v == 0 for v in scratch.values()), scratch


def _bodies(asm):
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, flags=re.M)
    out = {}
    for n in names:
        t = asm[asm.index("\n" + n + ":"):]
        out[int(re.search(r"k_scoreILi(\d)E", n).group(1))] = t[:t.index("s_endpgm")]
    return out


_FMA = r"\bv_fma_f64\b|\bv_fmac_f64\b"
PROBE = """#include <hip/hip_runtime.h>
extern "C" __global__ void probe_div(const double* a, double* o) { o[threadIdx.x] = __ddiv_rn(a[threadIdx.x], a[threadIdx.x + 64]); }
extern "C" __global__ void probe_sqrt(const double* a, double* o) { o[threadIdx.x] = __dsqrt_rn(a[threadIdx.x]); }
"""


@abi_util.needs_hipcc
def test_no_fma_outside_the_division_s_and_the_root_s_own_sequences(tmp_path):
    """-ffp-contract=off and the _rn intrinsics: L1_NORM and DOT_PRODUCT hold no double FMA at all.  A double division and a double square
    root are refinement sequences that use FMAs of their own; how many, a two-kernel probe built with the same flags tells.  Every other
    kernel holds exactly as many FMAs as its divisions (one v_div_fixup_f64 each) and roots (one v_rsq_f64 each) account for, and its
    products and sums are v_mul_f64 and v_add_f64."""
    from orb_slam3_modified_amd.build import FLAGS, SCORE_SOURCE
    body = _bodies(abi_util.device_asm(SCORE_SOURCE, hidden=True))
    src = tmp_path / "probe.hip"
    src.write_text(PROBE)
    out = tmp_path / "probe.s"
    flags = [f for f in FLAGS if f not in ("-shared", "-fPIC", "-ldl")]
    p = subprocess.run(["hipcc"] + flags + ["-S", "--cuda-device-only", "-o", str(out), str(src)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True)
    assert p.returncode == 0, p.stdout[-2000:]
    probe = out.read_text()
    pd = probe[probe.index("\nprobe_div:"):]
    pd = pd[:pd.index("s_endpgm")]
    ps = probe[probe.index("\nprobe_sqrt:"):]
    ps = ps[:ps.index("s_endpgm")]
    per_div, per_sqrt = len(re.findall(_FMA, pd)), len(re.findall(_FMA, ps))
    assert pd.count("v_div_fixup_f64") == 1 and ps.count("v_rsq_f64") == 1 and per_div > 0 and per_sqrt > 0
    assert "v_rsq_f64" not in pd and "v_div_fixup_f64" not in ps
    for s in (0, 5):
        assert not re.findall(_FMA, body[s]) and "v_div_fixup_f64" not in body[s] and "v_rsq_f64" not in body[s], s
    for s in (1, 2, 4):
        ndiv, nsqrt = body[s].count("v_div_fixup_f64"), body[s].count("v_rsq_f64")
        assert len(re.findall(_FMA, body[s])) == ndiv * per_div + nsqrt * per_sqrt, (s, ndiv, nsqrt, per_div, per_sqrt)
    assert body[1].count("v_rsq_f64") > 0 and "v_div_fixup_f64" not in body[1]          # L2: the final root only
    assert body[2].count("v_div_fixup_f64") > 0 and "v_rsq_f64" not in body[2]          # chi-square: the quotient only
    assert body[4].count("v_rsq_f64") > 0 and "v_div_fixup_f64" not in body[4]          # Bhattacharyya: the per-word root only
    for s in (1, 2, 4, 5):
        assert "v_mul_f64" in body[s] and "v_add_f64" in body[s], s
    assert "v_add_f64" in body[0]
    for s, b in body.items():
        assert not re.search(r"v_fma_f32|v_fmac_f32|v_mad_f32|v_pk_fma", b), s


@abi_util.needs_hipcc
def test_the_kernel_s_shape():
    """The query is staged by 16-byte loads into 16-byte LDS stores, the terms leave their lanes by v_readlane in the ballot's order, nothing
    is a flat access or an atomic, and the LDS block is the staged query's."""
    from orb_slam3_modified_amd import score
    from orb_slam3_modified_amd.build import SCORE_SOURCE
    asm = abi_util.device_asm(SCORE_SOURCE, hidden=True)
    assert "flat_load" not in asm and "flat_store" not in asm and "atomic" not in asm.split(".amdgpu_metadata")[0]
    for s, b in _bodies(asm).items():
        assert "global_load_dwordx4" in b and "ds_write_b128" in b and "v_readlane_b32" in b and "s_ff1_i32_b64" in b, s
    lds = set(map(int, re.findall(r"^\s*\.amdhsa_group_segment_fixed_size\s+(\d+)", asm, flags=re.M)))
    assert lds == {(score.QUERY_LDS + 4) * 4 + (score.QUERY_LDS + 2) * 8} and max(lds) <= 65536
