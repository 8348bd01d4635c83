"""include/orbx_mpdesc.h <-> liborbx_mpdesc.so: the batched ComputeDistinctiveDescriptors is a library of its own beside the product
(CPU-only checks)."""
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
HEADER = "orbx_mpdesc.h"
NAMES = ("create", "destroy", "last_error", "select_device", "select")


def test_build_produces_the_mpdesc_library():
    from orb_slam3_modified_amd import _lib, build
    build.build()
    assert os.path.isfile(build.MPDESC_OUT) and build.MPDESC_OUT == _lib.MPDESC_LIB_PATH
    assert os.path.dirname(build.MPDESC_OUT) == os.path.dirname(_lib.LIB_PATH) == os.path.join(ROOT, "orb_slam3_modified_amd")
    assert os.path.basename(build.MPDESC_OUT) == "liborbx_mpdesc.so"
    assert HEADER in build.HEADERS
    rec = [l for l in build.LIBS if l.out == build.MPDESC_OUT]
    assert len(rec) == 1 and rec[0].sources == (build.MPDESC_SOURCE,) and rec[0].hidden and rec[0].product


def test_mpdesc_library_exports_exactly_its_header():
    from orb_slam3_modified_amd import _lib, build
    build.build()
    names = _declared(HEADER)
    assert names == sorted("orbx_mpdesc_" + n for n in NAMES), names
    exported = _exported(_lib.MPDESC_LIB_PATH)
    assert {e for e in exported if e.startswith("orbx_")} == set(names)
    assert not [e for e in exported if not e.startswith("orbx_mpdesc_") and not e.startswith("_")], sorted(exported)[:10]   # -fvisibility=hidden


def test_product_library_keeps_its_abi_and_its_kernels():
    from orb_slam3_modified_amd import _lib, build
    build.build()
    names = set(_declared(HEADER))
    for other in (_lib.LIB_PATH, _lib.FUSE_LIB_PATH, _lib.TRIMATCH_LIB_PATH, _lib.MATCH_LIB_PATH, _lib.INITMATCH_LIB_PATH, _lib.BOW_LIB_PATH,
                  _lib.STEREO_LIB_PATH):
        assert not names & _exported(other), other
    assert not names & set(_declared("orbx.h"))
    assert len(_declared("orbx.h")) == 100
    assert build.kernels_hash() == KERNELS_HASH
    assert os.path.dirname(build.MPDESC_SOURCE) == "mpdesc" and "orbx_mpdesc.hip" not in os.listdir(build.CSRC)
    src = open(os.path.join(build.CSRC, build.MPDESC_SOURCE)).read()
    assert "side/orbx_handle.h" in src and "side/orbx_pair_device.h" in src and "orbx_internal.h" not in src


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not installed")
def test_the_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "orbx_mpdesc.h"\n'
                   "typedef char obs_is_8_bytes[sizeof(orbx_mpdesc_obs) == 8 ? 1 : -1];\n"
                   "typedef char side_is_24_bytes[sizeof(orbx_mpdesc_side) == 24 ? 1 : -1];\n"
                   "typedef char the_limit[ORBX_MPDESC_MAX_OBS == 1024 ? 1 : -1];\n"
                   "int main(void) { orbx_mpdesc_obs o = {0, 0}; return o.frame + o.row; }\n")
    obj = tmp_path / "use.o"
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(obj)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-2000:]


def test_python_binding_covers_the_header():
    from orb_slam3_modified_amd import _lib, build
    build.build()
    M = _lib.mpdesc_lib()
    assert set(M._orbx_mpdesc_symbols) == set(_declared(HEADER))
    from orb_slam3_modified_amd import mpdesc
    assert issubclass(mpdesc.DistinctBatch, _lib.SideHandle)
    for m in ("select_device", "select", "close"):
        assert callable(getattr(mpdesc.DistinctBatch, m))
    assert mpdesc.DistinctResult._fields == ("best", "median", "desc")
    # the structures the binding passes are the header's: the same fields, in order and size
    assert abi_util.struct_fields(HEADER, "orbx_mpdesc_side") == [f for f, _ in _lib.OrbxMpdescSide._fields_]
    assert C.sizeof(_lib.OrbxMpdescSide) == 2 * 8 + 2 * 4
    assert abi_util.struct_fields(HEADER, "orbx_mpdesc_obs") == list(mpdesc.OBS_DTYPE.names) and mpdesc.OBS_DTYPE.itemsize == 8
    # the constants the binding states are the library's
    src = open(os.path.join(build.CSRC, build.MPDESC_SOURCE)).read()
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert "#define ORBX_MPDESC_MAX_OBS %d\n" % mpdesc.MAX_OBS in text
    for line in ("kSmallCap = %d;" % mpdesc.SMALL_CAP, "kMidCap = %d;" % mpdesc.MID_CAP, "kChunk = %d;" % mpdesc.POINTS_PER_WORKGROUP,
                 "kLanes = %d;" % mpdesc.LANES_PER_PASS, "small_max = kSmallCap, mid_max = kMidCap;",
                 'env_int("ORBX_MPDESC_SMALL_MAX", 0, kSmallCap, kSmallCap)', 'env_int("ORBX_MPDESC_MID_MAX", 0, kMidCap, kMidCap)'):
        assert line in src, line
    assert (mpdesc.SMALL_MAX, mpdesc.MID_MAX) == (mpdesc.SMALL_CAP, mpdesc.MID_CAP) and mpdesc.MID_CAP < mpdesc.MAX_OBS < 2048
    # the header states the specification's corners and what is out of scope
    for word in ("(int)(0.5 * (N - 1))", "strict <", "the lower middle", "mObservations", "two-camera rig", "d_best[m] = -2", "not touched",
                 "ORBX_MPDESC_SMALL_MAX", "ORBX_MPDESC_MID_MAX", "near N = 1400"):
        assert word in text, word


def test_bad_arguments_are_rejected_without_a_device():
    """Argument checks that come before any device call, all three forms."""
    from orb_slam3_modified_amd import _lib
    M = _lib.mpdesc_lib()
    h = C.c_void_p(0)
    assert M.orbx_mpdesc_create(None, 0) == _lib.ORBX_E_INVALID
    assert b"null" in M.orbx_mpdesc_last_error(None)
    assert M.orbx_mpdesc_create(C.byref(h), -1) == _lib.ORBX_E_INVALID and not h.value
    assert b"device" in M.orbx_mpdesc_last_error(None)
    side = _lib.OrbxMpdescSide()
    for s in (side, None):
        r = None if s is None else C.byref(s)
        assert M.orbx_mpdesc_select_device(None, r, None, 1, None, 1, None, None, 1, None, None, None) == _lib.ORBX_E_INVALID
        assert M.orbx_mpdesc_select(None, r, None, 1, None, 1, None, None, 1, None, None) == _lib.ORBX_E_INVALID
    M.orbx_mpdesc_destroy(None)


@abi_util.needs_hipcc
def test_mpdesc_kernels_compile_without_scratch():
    from orb_slam3_modified_amd.build import MPDESC_SOURCE
    scratch = abi_util.kernel_scratch(MPDESC_SOURCE, hidden=True)
    assert len([n for n in scratch if "k_mpd_point" in n]) == 2        # the LDS-matrix instantiation and the recomputing one
    assert len([n for n in scratch if "k_mpd_small" in n]) == 1 and len([n for n in scratch if "k_mpd_classify" in n]) == 1 and len(scratch) == 4
    assert all(v == 0 for v in scratch.values()), scratch


@abi_util.needs_hipcc
def test_the_forms_keep_their_work_in_lds():
    """Nothing is a flat access; the lane-per-observation form and the matrix form keep their rows in LDS as halfwords and read descriptors
    16 bytes at a time; the recomputing form stores no row; the static and dynamic LDS blocks stay within what the other side libraries
    use."""
    from orb_slam3_modified_amd.build import CSRC, MPDESC_SOURCE
    asm = abi_util.device_asm(MPDESC_SOURCE, hidden=True)
    assert "flat_load" not in asm and "flat_store" not in asm and "flat_atomic" not in asm

    def body(name):
        t = asm[asm.index(name + ":"):] if name + ":" in asm else asm[asm.index(name):]
        return t[:t.index("s_endpgm")]
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, flags=re.M)
    small, = [n for n in names if "k_mpd_small" in n]
    matrix, = [n for n in names if "k_mpd_pointILb1E" in n]
    recompute, = [n for n in names if "k_mpd_pointILb0E" in n]
    for n in (small, matrix):
        assert "ds_write_b16" in body(n) and "ds_read_u16" in body(n) and "ds_read_b128" in body(n) and "v_bcnt_u32_b32" in body(n), n
    assert "ds_write_b16" not in body(recompute) and "ds_read_b128" in body(recompute) and "ds_min_i32" in body(recompute)
    lds = dict(zip(names, map(int, re.findall(r"^\s*\.amdhsa_group_segment_fixed_size\s+(\d+)", asm, flags=re.M))))
    assert 32768 + 12288 <= lds[small] <= 65536
    src = open(os.path.join(CSRC, MPDESC_SOURCE)).read()
    assert "kMidLds <= 155648" in src and 256 * 32 + 256 * 256 * 2 <= 155648
