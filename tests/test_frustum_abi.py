"""include/orbx_frustum.h <-> liborbx_frustum.so: the batched Frame::isInFrustum is a library of its own beside the product (CPU-only
checks)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import abi_util
from tests.abi_util import declared as _declared, exported as _exported

ROOT = abi_util.ROOT
KERNELS_HASH = "cfa5f580d25d496f"   # the product's kernel sources: this library changes none of them
HEADER = "orbx_frustum.h"
NAMES = ("create", "destroy", "last_error", "level_thresholds", "project_device", "project", "project_reference")


def _fields(name: str) -> list:
    """(field, array length or 1) of `typedef struct <name> { ... }` in the header, in order (abi_util.struct_fields knows no arrays)."""
    h = open(os.path.join(ROOT, "include", HEADER)).read()
    body = re.sub(r"/\*.*?\*/", "", h[h.index("typedef struct %s {" % name):h.index("} %s;" % name)], flags=re.S)
    return [(n, int(k or 1)) for decl in re.findall(r"float\s+([^;]+);", body) for n, k in re.findall(r"(\w+)(?:\[(\d+)\])?\s*(?:,|$)", decl.strip())]


def test_build_produces_the_frustum_library():
    from orb_slam3_modified_amd import _lib, build
    build.build()
    assert os.path.isfile(build.FRUSTUM_OUT) and build.FRUSTUM_OUT == _lib.FRUSTUM_LIB_PATH
    assert os.path.dirname(build.FRUSTUM_OUT) == os.path.dirname(_lib.LIB_PATH) == os.path.join(ROOT, "orb_slam3_modified_amd")
    assert os.path.basename(build.FRUSTUM_OUT) == "liborbx_frustum.so" and HEADER in build.HEADERS
    rec = [l for l in build.LIBS if l.out == build.FRUSTUM_OUT]
    assert len(rec) == 1 and rec[0].sources == (build.FRUSTUM_SOURCE,) and rec[0].hidden and not rec[0].product
    assert "-ffp-contract=off" in build.FLAGS                      # no product and sum, and no product and difference, is fused
    assert not [f for f in build.FLAGS if "fast" in f or "correctly-rounded" in f or "unsafe" in f or "denormal" in f], build.FLAGS


def test_frustum_library_exports_exactly_its_header():
    from orb_slam3_modified_amd import _lib, build
    build.build()
    names = _declared(HEADER)
    assert names == sorted("orbx_frustum_" + n for n in NAMES), names
    exported = _exported(_lib.FRUSTUM_LIB_PATH)
    assert {e for e in exported if e.startswith("orbx_")} == set(names)
    assert not [e for e in exported if not e.startswith("orbx_frustum_") and not e.startswith("_")], sorted(exported)[:10]   # -fvisibility=hidden
    needed = subprocess.check_output(["readelf", "-d", _lib.FRUSTUM_LIB_PATH]).decode()
    assert "liborbx" not in needed                                 # it takes nothing from the product or from the matcher it feeds


def test_every_other_library_keeps_its_abi_and_the_product_its_kernels():
    from orb_slam3_modified_amd import build
    build.build()
    names = set(_declared(HEADER))
    others = [l.out for l in build.LIBS if l.out != build.FRUSTUM_OUT]
    assert len(others) == len(build.LIBS) - 1
    for other in others:
        assert not names & _exported(other), other
    for header in build.HEADERS:
        if header != HEADER:
            assert not names & set(_declared(header)), header
    assert len(_declared("orbx.h")) == 100 and build.kernels_hash() == KERNELS_HASH
    assert len(_declared("orbx_localmatch.h")) == 5
    assert os.path.dirname(build.FRUSTUM_SOURCE) == "frustum" and "orbx_frustum.hip" not in os.listdir(build.CSRC)
    src = open(os.path.join(build.CSRC, build.FRUSTUM_SOURCE)).read()
    assert "side/orbx_handle.h" in src and "orbx_internal.h" not in src
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code and not re.search(r"atomic\w*\s*\(\s*\(?\s*(float|double)", code)
    assert code.count("project_one<") == 3 and "log(" not in code[code.index("__global__"):]   # one statement of the specification; no log on the device


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not installed")
def test_the_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "orbx_frustum.h"\nint main(void) { orbx_frustum_point p; orbx_frustum_item i; return (int)sizeof(p) + (int)sizeof(i); }\n'
                   'typedef char point_is_48[sizeof(orbx_frustum_point) == 48 ? 1 : -1];\n'
                   'typedef char item_is_112[sizeof(orbx_frustum_item) == 112 ? 1 : -1];\n'
                   'typedef char row_is_32[sizeof(orbx_localmatch_point) == 32 ? 1 : -1];\n')
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "use.o")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-2000:]


def test_python_binding_covers_the_header():
    from orb_slam3_modified_amd import _lib, build
    build.build()
    M = _lib.frustum_lib()
    assert set(M._orbx_frustum_symbols) == set(_declared(HEADER))
    from orb_slam3_modified_amd import frustum, localmatch
    assert issubclass(frustum.FrustumBatch, _lib.SideHandle)
    for m in ("project", "project_host"):
        assert callable(getattr(frustum.FrustumBatch, m))
    assert callable(frustum.reference) and callable(frustum.level_thresholds)
    # the records the binding passes are the header's: the same fields, in order and size
    for struct, dtype, size in (("orbx_frustum_point", frustum.TABLE_DTYPE, 48), ("orbx_frustum_item", frustum.ITEM_DTYPE, 112)):
        assert _fields(struct) == [(n, int(np.prod(dtype[n].shape, dtype=int))) for n in dtype.names] and dtype.itemsize == size, _fields(struct)
    assert frustum.ITEM_DTYPE.fields["far_th"][1] == 24 * 4 and frustum.TABLE_DTYPE.fields["max_dist"][1] == 32
    assert frustum.POINT_DTYPE is localmatch.POINT_DTYPE
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    for name, value in (("SUM_LTR", 0), ("SUM_TREE", 1), ("LOG_DOUBLE", 0), ("LOG_FLOAT", 1), ("MAX_LEVELS", 16)):
        assert re.search(r"#define ORBX_FRUSTUM_%s %d\b" % (name, value), text) and getattr(frustum, name) == value
    # the header states what is out of scope, what is not settled and what is undefined
    for word in ("isInFrustumChecks", "KannalaBrandt8", "ProjectPointDistort", "has not been settled", "Limits", "x86", "0x1.333332p+0",
                 "0x1.333334p+0", "monotone", "4096", "never inverts"):
        assert word in text, word


def test_bad_arguments_are_rejected_without_a_device():
    """Argument checks that come before any device call, all forms; the host twin and the thresholds need no device at all."""
    from orb_slam3_modified_amd import _lib, frustum
    M = _lib.frustum_lib()
    h = C.c_void_p(0)
    assert M.orbx_frustum_create(None, 0) == _lib.ORBX_E_INVALID
    assert b"null" in M.orbx_frustum_last_error(None)
    assert M.orbx_frustum_create(C.byref(h), -1) == _lib.ORBX_E_INVALID and not h.value
    assert b"device" in M.orbx_frustum_last_error(None)
    args = (None, None, 1, None, 1, None, None, 8, 0.18, 8, 0.5, 0, 0, None, None, None)
    assert M.orbx_frustum_project_device(None, *args, None) == _lib.ORBX_E_INVALID
    assert M.orbx_frustum_project(None, *args) == _lib.ORBX_E_INVALID
    M.orbx_frustum_destroy(None)
    # the host twin runs the same checks as the two device forms (one function) and reports the reason
    pts, obs = np.zeros(4, frustum.TABLE_DTYPE), np.zeros(4, np.int32)
    items, idx, nmp = np.zeros(2, frustum.ITEM_DTYPE), np.zeros((2, 8), np.int32), np.zeros(2, np.int32)
    mp, ntm = np.zeros((2, 8), frustum.POINT_DTYPE), np.zeros(2, np.int32)
    p = _lib.ptr

    def call(points=pts, obs_=obs, npoints=4, items_=items, nitems=2, idx_=idx, nmp_=nmp, mcap=8, lsf=0.18, nlevels=8, cos=0.5, order=0, kind=0,
             mp_=mp, ntomatch=ntm):
        return M.orbx_frustum_project_reference(p(points), p(obs_), npoints, p(items_), nitems, p(idx_), p(nmp_), mcap, lsf, nlevels, cos, order,
                                                kind, p(mp_), None, p(ntomatch))
    assert call() == _lib.ORBX_OK and list(ntm) == [0, 0]
    for kw, word in ((dict(points=None), b"null"), (dict(obs_=None), b"null"), (dict(items_=None), b"null"), (dict(idx_=None), b"null"),
                     (dict(nmp_=None), b"null"), (dict(mp_=None), b"null"), (dict(ntomatch=None), b"null"), (dict(npoints=0), b"at least 1"),
                     (dict(nitems=0), b"at least 1"), (dict(mcap=0), b"at least 1"), (dict(nlevels=0), b"nlevels"), (dict(nlevels=17), b"nlevels"),
                     (dict(order=2), b"sum_order"), (dict(kind=-1), b"log_kind"), (dict(cos=float("nan")), b"cos_limit"),
                     (dict(nitems=1 << 20, mcap=1 << 12), b"INT_MAX")):
        assert call(**kw) == _lib.ORBX_E_INVALID, kw
        assert word in M.orbx_frustum_last_error(None), (kw, M.orbx_frustum_last_error(None))
    src = open(os.path.join(ROOT, "orb_slam3_modified_amd", "csrc", "frustum", "orbx_frustum.hip")).read()
    assert src.count("call_problem(") == 4 and "16-byte aligned" in src and "same_device(" in src   # what only the device form can check


@abi_util.needs_hipcc
def test_frustum_kernels_compile_without_scratch():
    from orb_slam3_modified_amd.build import FRUSTUM_SOURCE
    scratch = abi_util.kernel_scratch(FRUSTUM_SOURCE, hidden=True)
    assert len([n for n in scratch if "k_frustum" in n]) == 3 and len(scratch) == 3      # the check and one projection per sum order
    assert all(v == 0 for v in scratch.values()), scratch


@abi_util.needs_hipcc
def test_the_projection_kernel_reads_its_item_through_scalar_loads():
    """The item's constants and the thresholds are wave-uniform: scalar loads, not a load per lane.  A lane's own traffic is the index,
    the observations, its record (two 16-byte loads and max_dist), two 16-byte stores and the depth; one integer atomic per wave; nothing
    is a flat access.  That no product is fused with the sum or the difference after it is the GPU test's to show, bit for bit."""
    from orb_slam3_modified_amd.build import FRUSTUM_SOURCE
    asm = abi_util.device_asm(FRUSTUM_SOURCE, hidden=True)
    assert "flat_load" not in asm and "flat_store" not in asm and "flat_atomic" not in asm
    for inst in ("k_frustumILb0EE", "k_frustumILb1EE"):
        k = asm[asm.index(inst):]
        k = k[:k.index("s_endpgm")]
        assert len(re.findall(r"global_load_dwordx4", k)) == 2 and len(re.findall(r"global_store_dwordx4", k)) == 2, inst
        assert len(re.findall(r"\bglobal_load_dword\b", k)) == 4, inst          # ntomatch[b], idx, obs, and max_dist: the padding is not fetched
        assert len(re.findall(r"\bglobal_store_dword\b", k)) == 1, inst         # depth
        assert len(re.findall(r"global_atomic_add\b", k)) == 1 and "global_atomic_add_f32" not in k, inst
        scalar_dwords = sum({"": 1, "x2": 2, "x4": 4, "x8": 8, "x16": 16}[w] for w in re.findall(r"s_load_dword(x\d+)?\b", k))
        assert scalar_dwords >= 25 + 15, (inst, scalar_dwords)                  # the item and the thresholds
        assert "s_bcnt1_i32_b64" in k                                           # the ballot's popcount
        # five correctly rounded divisions (invz, u, v, viewCos, ratio) and two square roots; their expansions hold the only fused operations
        assert len(re.findall(r"v_div_fixup_f32", k)) == 5 and len(re.findall(r"v_sqrt_f32", k)) == 2, inst
