"""include/orbx_placeindex.h <-> liborbx_placeindex.so: place recognition through a device inverted file is a library of its own beside the
product and beside liborbx_place.so, with which it shares csrc/place/orbx_place_kernels.h (CPU-only checks)."""
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
HEADER = "orbx_placeindex.h"
NAMES = ("create", "destroy", "last_error", "sync_device", "query_device", "query")
SHARED = ("struct Work {", "void place_pair_wave(", "void k_place_check(", "void k_place_members(", "void k_place_scan(", "void k_place_select(",
          "int rank_of(")


def test_build_produces_the_placeindex_library():
    from orb_slam3_modified_amd import _lib, build
    build.build()
    assert os.path.isfile(build.PLACEINDEX_OUT) and build.PLACEINDEX_OUT == _lib.PLACEINDEX_LIB_PATH
    assert os.path.dirname(build.PLACEINDEX_OUT) == os.path.dirname(_lib.LIB_PATH) == os.path.join(ROOT, "orb_slam3_modified_amd")
    assert os.path.basename(build.PLACEINDEX_OUT) == "liborbx_placeindex.so" and HEADER in build.HEADERS
    rec = [l for l in build.LIBS if l.out == build.PLACEINDEX_OUT]
    assert len(rec) == 1 and rec[0].sources == (build.PLACEINDEX_SOURCE,) and rec[0].hidden and not rec[0].product
    place = [l for l in build.LIBS if l.out == build.PLACE_OUT][0]
    assert rec[0].deps == place.deps == (build.PLACE_KERNELS,) and os.path.isfile(os.path.join(build.CSRC, build.PLACE_KERNELS))
    assert "-ffp-contract=off" in build.FLAGS


def test_placeindex_library_exports_exactly_its_header():
    from orb_slam3_modified_amd import _lib, build
    build.build()
    names = _declared(HEADER)
    assert names == sorted("orbx_placeindex_" + n for n in NAMES), names
    exported = _exported(_lib.PLACEINDEX_LIB_PATH)
    assert {e for e in exported if e.startswith("orbx_")} == set(names)
    assert not [e for e in exported if not e.startswith("orbx_placeindex_") and not e.startswith("_")], sorted(exported)[:10]   # -fvisibility=hidden
    needed = subprocess.check_output(["readelf", "-d", _lib.PLACEINDEX_LIB_PATH]).decode()
    assert "liborbx.so" not in needed and "liborbx_place.so" not in needed          # it takes nothing from the product or from the dense library


def test_every_other_library_keeps_its_abi_and_the_product_its_kernels():
    from orb_slam3_modified_amd import build
    build.build()
    names = set(_declared(HEADER))
    others = [l.out for l in build.LIBS if l.out != build.PLACEINDEX_OUT]
    assert len(others) == len(build.LIBS) - 1
    for other in others:
        assert not names & _exported(other), other
    for header in build.HEADERS:
        if header != HEADER:
            assert not names & set(_declared(header)), header
    assert len(_declared("orbx.h")) == 100 and build.kernels_hash() == KERNELS_HASH
    assert len(_declared("orbx_place.h")) == 5
    assert os.path.dirname(build.PLACEINDEX_SOURCE) == "placeindex" and "orbx_placeindex.hip" not in os.listdir(build.CSRC)


def test_the_two_place_libraries_share_one_query_path():
    """What comes after membership is stated once, in csrc/place/orbx_place_kernels.h, and both sources include it."""
    from orb_slam3_modified_amd import build
    shared = open(os.path.join(build.CSRC, build.PLACE_KERNELS)).read()
    dense = open(os.path.join(build.CSRC, build.PLACE_SOURCE)).read()
    index = open(os.path.join(build.CSRC, build.PLACEINDEX_SOURCE)).read()
    for text in SHARED:
        assert text in shared and text not in dense and text not in index, text
    assert '#include "orbx_place_kernels.h"' in dense and '#include "../place/orbx_place_kernels.h"' in index
    assert "side/orbx_handle.h" in index and "side/orbx_bowvec_device.h" in index and "orbx_internal.h" not in index
    for src in (shared, index):
        code = re.sub(r"//.*", "", src)
        assert "asm" not in code
        assert not re.search(r"atomic\w*\s*\(\s*\(?\s*(float|double)", code)
    assert "atomicAdd" not in shared                      # the dense library adds nothing atomically; the file's counters are the index's alone
    for launch in ("k_place_check", "k_place_members", "k_place_scan", "k_place_select", "k_index_count", "k_index_tail", "k_index_score"):
        assert "hipLaunchKernelGGL(%s," % launch in index, launch


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not installed")
def test_the_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "orbx_placeindex.h"\nint main(void) { orbx_placeindex* p = 0; orbx_place_db d; (void)p; (void)d; return 0; }\n'
                   "typedef char the_bound[ORBX_PLACEINDEX_MAX_WORDS >= (1 << 20) && ORBX_PLACEINDEX_MAX_WORDS == (1 << 24) ? 1 : -1];\n")
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "use.o")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-2000:]


def test_python_binding_covers_the_header():
    import orb_slam3_modified_amd
    from orb_slam3_modified_amd import _lib, build, placeindex
    build.build()
    P = _lib.placeindex_lib()
    assert set(P._orbx_placeindex_symbols) == set(_declared(HEADER))
    assert orb_slam3_modified_amd.PlaceIndex is placeindex.PlaceIndex and issubclass(placeindex.PlaceIndex, _lib.SideHandle)
    for m in ("sync_device", "query_device", "query", "close"):
        assert callable(getattr(placeindex.PlaceIndex, m))
    src = open(os.path.join(build.CSRC, build.PLACEINDEX_SOURCE)).read()
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    group_shift = placeindex.COUNT_GROUP.bit_length() - 1
    for line in ("kScanTile = %d;" % placeindex.SCAN_TILE, "kGroupShift = %d;" % group_shift, 'env_int("ORBX_PLACE_LDS", 0, kPlaceLds, kPlaceLds)',
                 'env_int("ORBX_PLACEINDEX_SCAN_TILE", 2, kScanTile, kScanTile)', 'env_int("ORBX_PLACEINDEX_GROUP", 1, 64, 1 << kGroupShift)'):
        assert line in src, line
    assert "#define ORBX_PLACEINDEX_MAX_WORDS (1 << 24)" in text and placeindex.MAX_WORDS == 1 << 24
    for word in ("ORBX_PLACEINDEX_SCAN_TILE (2 .. %d)" % placeindex.SCAN_TILE, "BIT-IDENTICAL", "TAIL", "d_ncand = -1", "never returned",
                 "no result depends on it", "left\n * unsynced"):
        assert word in text, word


def test_bad_arguments_are_rejected_without_a_device():
    """Argument checks that come before any device call."""
    from orb_slam3_modified_amd import _lib
    P = _lib.placeindex_lib()
    h = C.c_void_p(0)
    assert P.orbx_placeindex_create(None, 0, 16) == _lib.ORBX_E_INVALID and b"null" in P.orbx_placeindex_last_error(None)
    assert P.orbx_placeindex_create(C.byref(h), -1, 16) == _lib.ORBX_E_INVALID and not h.value and b"device" in P.orbx_placeindex_last_error(None)
    for n_words in (0, -1, (1 << 24) + 1):
        assert P.orbx_placeindex_create(C.byref(h), 0, n_words) == _lib.ORBX_E_INVALID and not h.value
        assert b"n_words" in P.orbx_placeindex_last_error(None)
    assert P.orbx_placeindex_sync_device(None, None, None) == _lib.ORBX_E_INVALID
    assert P.orbx_placeindex_query_device(None, 0, 0, None, None, 1, None, None, None, None, None, None) == _lib.ORBX_E_INVALID
    assert P.orbx_placeindex_query(None, 0, 0, None, None, 1, None, None, None, None, None) == _lib.ORBX_E_INVALID
    P.orbx_placeindex_destroy(None)


def test_host_form_fails_loudly_without_a_device():
    """No GPU here: the handle cannot be made, and the class raises instead of computing anything on the host."""
    torch = pytest.importorskip("torch")
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_placeindex.py runs the host form")
    from orb_slam3_modified_amd import OrbxError, placeindex
    with pytest.raises(OrbxError) as e:
        placeindex.PlaceIndex(16, 0)
    assert e.value.code == -3 and "orbx_placeindex_create" in str(e.value)


@abi_util.needs_hipcc
def test_placeindex_kernels_compile_without_scratch_and_without_float_atomics():
    from orb_slam3_modified_amd import place
    from orb_slam3_modified_amd.build import PLACEINDEX_SOURCE
    scratch = abi_util.kernel_scratch(PLACEINDEX_SOURCE, hidden=True)
    assert sorted(re.search(r"(k_[a-z]+_[a-z]+)", n).group(1) for n in scratch) == [
        "k_index_count", "k_index_hist", "k_index_scatter", "k_index_score", "k_index_stale", "k_index_tail", "k_place_check", "k_place_members",
        "k_place_scan", "k_place_select", "k_scan_add", "k_scan_tile"]
    assert all(v == 0 for v in scratch.values()), scratch
    asm = abi_util.device_asm(PLACEINDEX_SOURCE, hidden=True).split(".amdgpu_metadata")[0]
    assert not re.search(r"atomic_\w*(f32|f64)", asm) and "cmpswap" not in asm
    assert set(re.findall(r"global_atomic_(\w+)", asm)) == {"add", "umin", "smin", "or"}, set(re.findall(r"global_atomic_(\w+)", asm))   # integers
    assert not re.search(r"\bv_fma_f64\b|\bv_fmac_f64\b|v_fma_f32|v_fmac_f32|v_mad_f32", asm)          # every operation rounded once
    lds = sorted(map(int, re.findall(r"^\s*\.amdhsa_group_segment_fixed_size\s+(\d+)", asm, flags=re.M)))
    assert lds[-1] == (place.QUERY_LDS + 4) * 4 + (place.QUERY_LDS + 2) * 8 and lds[-1] <= 65536
