"""include/orbx_place.h <-> liborbx_place.so: the batched place recognition is a library of its own beside the product (CPU-only checks)."""
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
HEADER = "orbx_place.h"
NAMES = ("create", "destroy", "last_error", "query_device", "query")


def test_build_produces_the_place_library():
    from orb_slam3_modified_amd import _lib, build
    build.build()
    assert os.path.isfile(build.PLACE_OUT) and build.PLACE_OUT == _lib.PLACE_LIB_PATH
    assert os.path.dirname(build.PLACE_OUT) == os.path.dirname(_lib.LIB_PATH) == os.path.join(ROOT, "orb_slam3_modified_amd")
    assert os.path.basename(build.PLACE_OUT) == "liborbx_place.so" and HEADER in build.HEADERS
    rec = [l for l in build.LIBS if l.out == build.PLACE_OUT]
    assert len(rec) == 1 and rec[0].sources == (build.PLACE_SOURCE,) and rec[0].hidden and not rec[0].product
    assert "-ffp-contract=off" in build.FLAGS


def test_place_library_exports_exactly_its_header():
    from orb_slam3_modified_amd import _lib, build
    build.build()
    names = _declared(HEADER)
    assert names == sorted("orbx_place_" + n for n in NAMES), names
    exported = _exported(_lib.PLACE_LIB_PATH)
    assert {e for e in exported if e.startswith("orbx_")} == set(names)
    assert not [e for e in exported if not e.startswith("orbx_place_") and not e.startswith("_")], sorted(exported)[:10]   # -fvisibility=hidden


def test_every_other_library_keeps_its_abi_and_the_product_its_kernels():
    from orb_slam3_modified_amd import build
    build.build()
    names = set(_declared(HEADER))
    others = [l.out for l in build.LIBS if l.out != build.PLACE_OUT]
    assert len(others) == len(build.LIBS) - 1
    for other in others:
        assert not names & _exported(other), other
    for header in build.HEADERS:
        if header != HEADER:
            assert not names & set(_declared(header)), header
    assert len(_declared("orbx.h")) == 100 and build.kernels_hash() == KERNELS_HASH
    assert os.path.dirname(build.PLACE_SOURCE) == "place" and "orbx_place.hip" not in os.listdir(build.CSRC)
    src = open(os.path.join(build.CSRC, build.PLACE_SOURCE)).read()
    assert "side/orbx_handle.h" in src and "side/orbx_bowvec_device.h" in src and "orbx_internal.h" not in src
    assert "asm" not in re.sub(r"//.*", "", src) and "atomicAdd" not in src
    score = open(os.path.join(build.CSRC, build.SCORE_SOURCE)).read()
    assert "side/orbx_bowvec_device.h" in score                       # one staging routine and one search for both libraries


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not installed")
def test_the_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "orbx_place.h"\nint main(void) { orbx_place_db d; orbx_place_queries q; (void)d; (void)q; return 0; }\n'
                   "typedef char the_values[ORBX_PLACE_RELOC == 0 && ORBX_PLACE_NBEST == 1 && ORBX_PLACE_COV == 10 ? 1 : -1];\n"
                   "typedef char db_size[sizeof(orbx_place_db) == 6 * sizeof(void*) + 8 ? 1 : -1];\n")
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "use.o")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-2000:]


def test_python_binding_covers_the_header():
    import orb_slam3_modified_amd
    from orb_slam3_modified_amd import _lib, build, place
    build.build()
    P = _lib.place_lib()
    assert set(P._orbx_place_symbols) == set(_declared(HEADER))
    assert orb_slam3_modified_amd.PlaceBatch is place.PlaceBatch and issubclass(place.PlaceBatch, _lib.SideHandle)
    for m in ("query_device", "query", "close"):
        assert callable(getattr(place.PlaceBatch, m))
    assert abi_util.struct_fields(HEADER, "orbx_place_db") == [f for f, _ in _lib.OrbxPlaceDb._fields_]
    assert abi_util.struct_fields(HEADER, "orbx_place_queries") == [f for f, _ in _lib.OrbxPlaceQueries._fields_]
    assert (place.RELOC, place.NBEST, place.COV) == (0, 1, 10)
    src = open(os.path.join(build.CSRC, build.PLACE_SOURCE)).read()
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    for line in ("kPlaceLds = %d;" % place.QUERY_LDS, "kTile = %d;" % place.DB_PER_WORKGROUP, 'env_int("ORBX_PLACE_LDS", 0, kPlaceLds, kPlaceLds)'):
        assert line in src, line
    for word in ("ORBX_PLACE_LDS (0 .. %d)" % place.QUERY_LDS, "Out of scope", "isBad()", "never repeat", "mnRelocQuery(0)", "d_ncand = -1"):
        assert word in text, word


def test_bad_arguments_are_rejected_without_a_device():
    """Argument checks that come before any device call."""
    from orb_slam3_modified_amd import _lib
    P = _lib.place_lib()
    h = C.c_void_p(0)
    assert P.orbx_place_create(None, 0) == _lib.ORBX_E_INVALID and b"null" in P.orbx_place_last_error(None)
    assert P.orbx_place_create(C.byref(h), -1) == _lib.ORBX_E_INVALID and not h.value and b"device" in P.orbx_place_last_error(None)
    assert P.orbx_place_query_device(None, 0, 0, None, None, 1, None, None, None, None, None, None) == _lib.ORBX_E_INVALID
    assert P.orbx_place_query(None, 0, 0, None, None, 1, None, None, None, None, None) == _lib.ORBX_E_INVALID
    P.orbx_place_destroy(None)


def test_host_form_fails_loudly_without_a_device():
    """No GPU here: the handle cannot be made, and the class raises instead of computing anything on the host."""
    torch = pytest.importorskip("torch")
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_place.py runs the host form")
    from orb_slam3_modified_amd import OrbxError, place
    with pytest.raises(OrbxError) as e:
        place.PlaceBatch(0)
    assert e.value.code == -3 and "orbx_place_create" in str(e.value)


@abi_util.needs_hipcc
def test_place_kernels_compile_without_scratch_and_without_float_atomics():
    from orb_slam3_modified_amd import place
    from orb_slam3_modified_amd.build import PLACE_SOURCE
    scratch = abi_util.kernel_scratch(PLACE_SOURCE, hidden=True)
    assert sorted(re.search(r"(k_place_[a-z]+)", n).group(1) for n in scratch) == ["k_place_check", "k_place_members", "k_place_pairs",
                                                                                  "k_place_scan", "k_place_select"]
    assert all(v == 0 for v in scratch.values()), scratch
    asm = abi_util.device_asm(PLACE_SOURCE, hidden=True).split(".amdgpu_metadata")[0]
    assert not re.search(r"atomic_\w*(f32|f64|add)", asm) and "global_atomic_smin" in asm and "global_atomic_or" in asm
    assert not re.search(r"\bv_fma_f64\b|\bv_fmac_f64\b|v_fma_f32|v_fmac_f32|v_mad_f32", asm)          # every operation rounded once
    lds = sorted(map(int, re.findall(r"^\s*\.amdhsa_group_segment_fixed_size\s+(\d+)", asm, flags=re.M)))
    assert lds[-1] == (place.QUERY_LDS + 4) * 4 + (place.QUERY_LDS + 2) * 8 and lds[-1] <= 65536
