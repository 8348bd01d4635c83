"""include/orbx_initmatch.h <-> liborbx_initmatch.so: the batched SearchForInitialization is a library of its own beside the product (CPU-only
checks)."""
import ctypes as C
import os
import re

from tests import abi_util
from tests.abi_util import declared as _declared, exported as _exported

ROOT = abi_util.ROOT
KERNELS_HASH = "cfa5f580d25d496f"   # the product's kernel sources: this library changes none of them
HEADER = "orbx_initmatch.h"


def test_build_produces_the_initmatch_library():
    from orb_slam3_modified_amd import _lib, build
    build.build()
    assert os.path.isfile(build.INITMATCH_OUT) and build.INITMATCH_OUT == _lib.INITMATCH_LIB_PATH
    assert os.path.dirname(build.INITMATCH_OUT) == os.path.dirname(_lib.LIB_PATH) == os.path.join(ROOT, "orb_slam3_modified_amd")
    assert os.path.basename(build.INITMATCH_OUT) == "liborbx_initmatch.so"
    assert HEADER in build.HEADERS
    rec = [l for l in build.LIBS if l.out == build.INITMATCH_OUT]
    assert len(rec) == 1 and rec[0].sources == (build.INITMATCH_SOURCE,) and rec[0].hidden and rec[0].product


def test_initmatch_library_exports_exactly_its_header():
    from orb_slam3_modified_amd import _lib, build
    build.build()
    names = _declared(HEADER)
    assert len(names) == 5 and all(n.startswith("orbx_initmatch_") for n in names), names
    exported = _exported(_lib.INITMATCH_LIB_PATH)
    assert {e for e in exported if e.startswith("orbx_")} == set(names)
    assert not [e for e in exported if not e.startswith("orbx_initmatch_") and not e.startswith("_")], sorted(exported)[:10]   # -fvisibility=hidden


def test_product_library_keeps_its_abi_and_its_kernels():
    from orb_slam3_modified_amd import _lib, build
    build.build()
    names = set(_declared(HEADER))
    assert not names & _exported(_lib.LIB_PATH), "liborbx.so exports a batched SearchForInitialization entry point"
    assert not names & _exported(_lib.MATCH_LIB_PATH)
    assert not names & set(_declared("orbx.h"))
    assert len(_declared("orbx.h")) <= 100
    assert build.kernels_hash() == KERNELS_HASH
    assert os.path.dirname(build.INITMATCH_SOURCE) == "initmatch" and "orbx_initmatch.hip" not in os.listdir(build.CSRC)
    src = open(os.path.join(build.CSRC, build.INITMATCH_SOURCE)).read()
    assert "side/orbx_handle.h" in src and "orbx_internal.h" not in src


def test_python_binding_covers_the_header():
    from orb_slam3_modified_amd import _lib, build
    build.build()
    M = _lib.initmatch_lib()
    assert set(M._orbx_initmatch_symbols) == set(_declared(HEADER))
    from orb_slam3_modified_amd import initmatch
    assert issubclass(initmatch.InitMatchBatch, _lib.SideHandle)
    for m in ("pairs", "pairs_device"):
        assert callable(getattr(initmatch.InitMatchBatch, m))
    assert initmatch.InitSide and initmatch.InitResult
    # the structure the binding passes is the header's: the same fields, in order and size
    in_header = abi_util.struct_fields(HEADER, "orbx_initmatch_side")
    assert in_header == [f for f, _ in _lib.OrbxInitMatchSide._fields_], in_header
    assert C.sizeof(_lib.OrbxInitMatchSide) == 3 * 8 + 2 * 4
    # the sizing formula the binding states is the library's: EuRoC's capacity fits the LDS, the initialisation extractor's does not
    assert initmatch.lds_bytes(1024, 1024) <= initmatch.LDS_MAX < initmatch.lds_bytes(5024, 5024)


def test_bad_arguments_are_rejected_without_a_device():
    """Argument checks that come before any device call, both forms."""
    from orb_slam3_modified_amd import _lib
    M = _lib.initmatch_lib()
    h = C.c_void_p(0)
    assert M.orbx_initmatch_create(None, 0) == _lib.ORBX_E_INVALID
    assert b"null" in M.orbx_initmatch_last_error(None)
    assert M.orbx_initmatch_create(C.byref(h), -1) == _lib.ORBX_E_INVALID and not h.value
    assert b"device" in M.orbx_initmatch_last_error(None)
    side = _lib.OrbxInitMatchSide()
    good, inverted = (C.c_float * 4)(0, 0, 752, 480), (C.c_float * 4)(752, 0, 0, 480)
    dev, host = M.orbx_initmatch_pairs_device, M.orbx_initmatch_pairs
    for sa, sb, npairs, bounds, window in ((side, side, 1, good, 100), (None, None, 1, good, 100), (side, side, 0, good, 100),
                                           (side, side, 1, good, -1), (side, side, 1, inverted, 100), (side, side, 1, None, 100)):
        ra, rb = (None if sa is None else C.byref(sa)), (None if sb is None else C.byref(sb))
        assert dev(None, ra, rb, None, npairs, bounds, window, 0.9, 1, None, None, None, None, None) == _lib.ORBX_E_INVALID
        assert host(None, ra, rb, None, npairs, bounds, window, 0.9, 1, None, None, None, None) == _lib.ORBX_E_INVALID
    M.orbx_initmatch_destroy(None)


@abi_util.needs_hipcc
def test_initmatch_kernels_compile_without_scratch():
    from orb_slam3_modified_amd.build import INITMATCH_SOURCE
    scratch = abi_util.kernel_scratch(INITMATCH_SOURCE, hidden=True)
    hit = [n for n in scratch if "k_init_pairs" in n]
    assert len(hit) == 2 and len(scratch) == 2, sorted(scratch)      # the LDS instantiation and the global-memory one
    assert all(v == 0 for v in scratch.values()), scratch


@abi_util.needs_hipcc
def test_the_lds_instantiation_reads_lds():
    """One template instantiation per path: the LDS one stages descriptors by LDS-DMA, reads them with ds_ instructions and has no flat access."""
    from orb_slam3_modified_amd.build import INITMATCH_SOURCE
    asm = abi_util.device_asm(INITMATCH_SOURCE, hidden=True)
    assert "flat_load" not in asm and "flat_store" not in asm and "flat_atomic" not in asm
    lds = asm[asm.index("k_init_pairsILb1E"):]
    lds = lds[:lds.index("s_endpgm")]
    assert "global_load_lds_dwordx4" in lds and "ds_read_b128" in lds and "ds_read" in lds
    assert not re.search(r"\bflat_", lds)
