"""include/orbx_match.h <-> liborbx_match.so: the batched SearchByBoW is a library of its own beside the product (CPU-only checks)."""
import ctypes as C
import os

from tests import abi_util
from tests.abi_util import declared as _declared, exported as _exported

ROOT = abi_util.ROOT
KERNELS_HASH = "cfa5f580d25d496f"   # the product's kernel sources: this library changes none of them


def test_build_produces_the_match_library():
    from orb_slam3_modified_amd import _lib, build
    build.build()
    assert os.path.isfile(build.MATCH_OUT) and build.MATCH_OUT == _lib.MATCH_LIB_PATH
    assert os.path.dirname(build.MATCH_OUT) == os.path.dirname(_lib.LIB_PATH) == os.path.join(ROOT, "orb_slam3_modified_amd")
    assert os.path.basename(build.MATCH_OUT) == "liborbx_match.so"
    assert "orbx_match.h" in build.HEADERS
    rec = [l for l in build.LIBS if l.out == build.MATCH_OUT]
    assert len(rec) == 1 and rec[0].sources == (build.MATCH_SOURCE,) and rec[0].hidden and rec[0].product


def test_match_library_exports_exactly_its_header():
    from orb_slam3_modified_amd import _lib, build
    build.build()
    names = _declared("orbx_match.h")
    assert len(names) == 5 and all(n.startswith("orbx_match_") for n in names), names
    exported = _exported(_lib.MATCH_LIB_PATH)
    assert {e for e in exported if e.startswith("orbx_")} == set(names)
    assert not [e for e in exported if not e.startswith("orbx_match_") and not e.startswith("_")], sorted(exported)[:10]   # -fvisibility=hidden


def test_product_library_keeps_its_abi_and_its_kernels():
    from orb_slam3_modified_amd import _lib, build
    build.build()
    mnames = set(_declared("orbx_match.h"))
    assert not mnames & _exported(_lib.LIB_PATH), "liborbx.so exports a batched SearchByBoW entry point"
    assert not mnames & set(_declared("orbx.h"))
    assert len(_declared("orbx.h")) <= 100
    assert build.kernels_hash() == KERNELS_HASH
    assert os.path.dirname(build.MATCH_SOURCE) == "match" and "orbx_match.hip" not in os.listdir(build.CSRC)
    assert os.path.isfile(os.path.join(build.CSRC, "match", "orbx_match.hip"))


def test_python_binding_covers_the_header():
    from orb_slam3_modified_amd import _lib, build
    build.build()
    M = _lib.match_lib()
    assert set(M._orbx_match_symbols) == set(_declared("orbx_match.h"))
    from orb_slam3_modified_amd import match
    assert issubclass(match.MatchBatch, _lib.SideHandle)
    for m in ("bow_pairs", "bow_pairs_device"):
        assert callable(getattr(match.MatchBatch, m))
    # the structure the binding passes is the header's
    in_header = abi_util.struct_fields("orbx_match.h", "orbx_match_side")
    assert in_header == [f for f, _ in _lib.OrbxMatchSide._fields_], in_header
    assert C.sizeof(_lib.OrbxMatchSide) == 8 * 8 + 2 * 4


def test_bad_arguments_are_rejected_without_a_device():
    """Argument checks that come before any device call."""
    from orb_slam3_modified_amd import _lib
    M = _lib.match_lib()
    h = C.c_void_p(0)
    assert M.orbx_match_create(None, 0) == _lib.ORBX_E_INVALID
    assert b"null" in M.orbx_match_last_error(None)
    assert M.orbx_match_create(C.byref(h), -1) == _lib.ORBX_E_INVALID and not h.value
    assert b"device" in M.orbx_match_last_error(None)
    side = _lib.OrbxMatchSide()
    assert M.orbx_match_bow_pairs_device(None, C.byref(side), C.byref(side), None, 1, 0, 0.7, 1, None, None, None, None) == _lib.ORBX_E_INVALID
    assert M.orbx_match_bow_pairs_device(None, None, None, None, 0, 7, 0.7, 1, None, None, None, None) == _lib.ORBX_E_INVALID
    assert M.orbx_match_bow_pairs(None, None, None, None, 1, 0, 0.7, 1, None, None, None) == _lib.ORBX_E_INVALID
    M.orbx_match_destroy(None)


@abi_util.needs_hipcc
def test_match_kernels_compile_without_scratch():
    from orb_slam3_modified_amd.build import MATCH_SOURCE
    scratch = abi_util.kernel_scratch(MATCH_SOURCE, hidden=True)
    hit = [n for n in scratch if "k_match_pairs" in n]
    assert len(hit) == 2 and len(scratch) == 2, sorted(scratch)      # the LDS instantiation and the global-memory one
    assert all(v == 0 for v in scratch.values()), scratch


@abi_util.needs_hipcc
def test_the_lds_instantiation_reads_lds():
    """One template instantiation per path: the LDS one reads descriptors with ds_ instructions and has no flat access."""
    from orb_slam3_modified_amd.build import MATCH_SOURCE
    asm = abi_util.device_asm(MATCH_SOURCE, hidden=True)
    assert "flat_load" not in asm and "flat_store" not in asm
    lds = asm[asm.index("k_match_pairsILb1E"):]
    lds = lds[:lds.index("s_endpgm")]
    assert "ds_read_b128" in lds and "global_load_lds_dwordx4" in lds


@abi_util.needs_hipcc
def test_the_single_camera_kernel_keeps_its_resources():
    """k_match_pairs: no scratch, and 160 bytes of static LDS with LDS, 156 on the global path (the counters, the histogram, the three
    maxima).  A shared form of the kernel (profiles/bowpair_core_refactor.txt) has to keep these figures."""
    import re
    from orb_slam3_modified_amd.build import MATCH_SOURCE
    asm = abi_util.device_asm(MATCH_SOURCE, hidden=True)
    got = {}
    for sym, body in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)(.*?)\.end_amdhsa_kernel", asm, flags=re.M | re.S):
        got["lds" if "ILb1E" in sym else "global"] = tuple(int(re.search(r"\.amdhsa_%s\s+(\d+)" % k, body).group(1))
                                                           for k in ("private_segment_fixed_size", "group_segment_fixed_size"))
    assert got == {"lds": (0, 160), "global": (0, 156)}, got
