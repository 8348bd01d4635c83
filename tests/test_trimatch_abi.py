"""include/orbx_trimatch.h <-> liborbx_trimatch.so: the batched SearchForTriangulation is a library of its own beside the product (CPU-only
checks)."""
import ctypes as C
import os
import re

import numpy as np

from tests import abi_util
from tests.abi_util import declared as _declared, exported as _exported

ROOT = abi_util.ROOT
KERNELS_HASH = "cfa5f580d25d496f"   # the product's kernel sources: this library changes none of them
HEADER = "orbx_trimatch.h"


def test_build_produces_the_trimatch_library():
    from orb_slam3_modified_amd import _lib, build
    build.build()
    assert os.path.isfile(build.TRIMATCH_OUT) and build.TRIMATCH_OUT == _lib.TRIMATCH_LIB_PATH
    assert os.path.dirname(build.TRIMATCH_OUT) == os.path.dirname(_lib.LIB_PATH) == os.path.join(ROOT, "orb_slam3_modified_amd")
    assert os.path.basename(build.TRIMATCH_OUT) == "liborbx_trimatch.so"
    assert HEADER in build.HEADERS
    rec = [l for l in build.LIBS if l.out == build.TRIMATCH_OUT]
    assert len(rec) == 1 and rec[0].sources == (build.TRIMATCH_SOURCE,) and rec[0].hidden and rec[0].product
    assert "-ffp-contract=off" in build.FLAGS       # the gates' float expressions are not contracted


def test_trimatch_library_exports_exactly_its_header():
    from orb_slam3_modified_amd import _lib, build
    build.build()
    names = _declared(HEADER)
    assert names == sorted("orbx_trimatch_" + n for n in ("create", "destroy", "last_error", "pairs_device", "pairs")), names
    exported = _exported(_lib.TRIMATCH_LIB_PATH)
    assert {e for e in exported if e.startswith("orbx_")} == set(names)
    assert not [e for e in exported if not e.startswith("orbx_trimatch_") and not e.startswith("_")], sorted(exported)[:10]   # -fvisibility=hidden


def test_product_library_keeps_its_abi_and_its_kernels():
    from orb_slam3_modified_amd import _lib, build
    build.build()
    names = set(_declared(HEADER))
    for other in (_lib.LIB_PATH, _lib.MATCH_LIB_PATH, _lib.INITMATCH_LIB_PATH, _lib.BOW_LIB_PATH, _lib.STEREO_LIB_PATH):
        assert not names & _exported(other), other
    assert not names & set(_declared("orbx.h"))
    assert len(_declared("orbx.h")) == 100
    assert build.kernels_hash() == KERNELS_HASH
    assert os.path.dirname(build.TRIMATCH_SOURCE) == "trimatch" and "orbx_trimatch.hip" not in os.listdir(build.CSRC)
    src = open(os.path.join(build.CSRC, build.TRIMATCH_SOURCE)).read()
    assert "side/orbx_handle.h" in src and "side/orbx_pair_device.h" in src and "orbx_internal.h" not in src


def test_python_binding_covers_the_header():
    from orb_slam3_modified_amd import _lib, build
    build.build()
    M = _lib.trimatch_lib()
    assert set(M._orbx_trimatch_symbols) == set(_declared(HEADER))
    from orb_slam3_modified_amd import trimatch
    assert issubclass(trimatch.TriMatchBatch, _lib.SideHandle)
    for m in ("pairs", "pairs_device"):
        assert callable(getattr(trimatch.TriMatchBatch, m))
    assert trimatch.TriMatchSide and trimatch.TriMatchResult
    # the structure the binding passes is the header's: the same fields, in order and size
    in_header = abi_util.struct_fields(HEADER, "orbx_trimatch_side")
    assert in_header == [f for f, _ in _lib.OrbxTriMatchSide._fields_], in_header
    assert C.sizeof(_lib.OrbxTriMatchSide) == 9 * 8 + 2 * 4
    # orbx_match_side with d_valid renamed and d_uright added
    match_side = abi_util.struct_fields("orbx_match.h", "orbx_match_side")
    assert [f for f in in_header if f != "d_uright"] == [("d_has_point" if f == "d_valid" else f) for f in match_side]
    # the sizing formula the binding states is the library's: EuRoC's capacity fits the LDS, the initialisation extractor's does not
    assert trimatch.lds_bytes(1024, 1024) <= trimatch.LDS_MAX < trimatch.lds_bytes(5024, 5024)
    # the header states what is out of scope
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    for word in ("two-camera rigs", "KannalaBrandt8", "FMA"):
        assert word in text, word


def test_fundamental_is_the_textbook_product():
    from orb_slam3_modified_amd import trimatch
    assert "NOT pinned to Eigen" in trimatch.fundamental.__doc__
    K = np.array([[250.0, 0, 160], [0, 250, 120], [0, 0, 1]])
    F = trimatch.fundamental(K, np.eye(3), [1.0, 0.0, 0.0], K)
    assert F.dtype == np.float32 and F.shape == (9,)
    assert np.allclose(F, [0, 0, 0, 0, 0, -1 / 250, 0, 1 / 250, 0], atol=1e-9)       # the epipolar line of (x1, y1) is y = y1
    x1 = np.array([10.0, 20.0, 1.0])
    assert abs(x1 @ F.reshape(3, 3).astype(np.float64) @ np.array([99.0, 20.0, 1.0])) < 1e-9
    g = trimatch.geometry(F, (3.0, 4.0))
    assert g.shape == (12,) and g.dtype == np.float32 and g[9:].tolist() == [3.0, 4.0, 0.0]


def test_bad_arguments_are_rejected_without_a_device():
    """Argument checks that come before any device call, both forms."""
    from orb_slam3_modified_amd import _lib
    M = _lib.trimatch_lib()
    h = C.c_void_p(0)
    assert M.orbx_trimatch_create(None, 0) == _lib.ORBX_E_INVALID
    assert b"null" in M.orbx_trimatch_last_error(None)
    assert M.orbx_trimatch_create(C.byref(h), -1) == _lib.ORBX_E_INVALID and not h.value
    assert b"device" in M.orbx_trimatch_last_error(None)
    side = _lib.OrbxTriMatchSide()
    tab = (C.c_float * 16)(*([1.0] * 16))
    dev, host = M.orbx_trimatch_pairs_device, M.orbx_trimatch_pairs
    for s, npairs, nlevels in ((side, 1, 8), (None, 1, 8), (side, 0, 8), (side, 1, 0), (side, 1, 17)):
        r = None if s is None else C.byref(s)
        assert dev(None, r, r, None, npairs, None, tab, tab, nlevels, 0, 0, 1, None, None, None) == _lib.ORBX_E_INVALID
        assert host(None, r, r, None, npairs, None, tab, tab, nlevels, 0, 0, 1, None, None) == _lib.ORBX_E_INVALID
    M.orbx_trimatch_destroy(None)


@abi_util.needs_hipcc
def test_trimatch_kernels_compile_without_scratch():
    from orb_slam3_modified_amd.build import TRIMATCH_SOURCE
    scratch = abi_util.kernel_scratch(TRIMATCH_SOURCE, hidden=True)
    hit = [n for n in scratch if "k_tri_pairs" in n]
    assert len(hit) == 2 and len(scratch) == 2, sorted(scratch)      # the LDS instantiation and the global-memory one
    assert all(v == 0 for v in scratch.values()), scratch


@abi_util.needs_hipcc
def test_the_lds_instantiation_reads_lds():
    """One template instantiation per path: the LDS one stages descriptors by LDS-DMA, reads them with ds_ instructions and has no flat access;
    the double comparison is there as such."""
    from orb_slam3_modified_amd.build import TRIMATCH_SOURCE
    asm = abi_util.device_asm(TRIMATCH_SOURCE, hidden=True)
    assert "flat_load" not in asm and "flat_store" not in asm and "flat_atomic" not in asm
    lds = asm[asm.index("k_tri_pairsILb1E"):]
    lds = lds[:lds.index("s_endpgm")]
    assert "global_load_lds_dwordx4" in lds and "ds_read_b128" in lds
    assert not re.search(r"\bflat_", lds)
    assert "v_cvt_f64_f32" in lds and "v_mul_f64" in lds and re.search(r"v_cmp\w*_f64", lds)
