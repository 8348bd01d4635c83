"""include/orbx_rigbow.h <-> liborbx_rigbow.so: the rig SearchByBoW and the stacker are a library of their own beside the product and
beside liborbx_match.so (CPU-only checks)."""
import ctypes as C
import os

from tests import abi_util
from tests.abi_util import declared as _declared, exported as _exported

ROOT = abi_util.ROOT
KERNELS_HASH = "cfa5f580d25d496f"   # the product's kernel sources: this library changes none of them


def test_build_produces_the_rigbow_library():
    from orb_slam3_modified_amd import _lib, build
    build.build()
    assert os.path.isfile(build.RIGBOW_OUT) and build.RIGBOW_OUT == _lib.RIGBOW_LIB_PATH
    assert os.path.dirname(build.RIGBOW_OUT) == os.path.dirname(_lib.LIB_PATH) == os.path.join(ROOT, "orb_slam3_modified_amd")
    assert os.path.basename(build.RIGBOW_OUT) == "liborbx_rigbow.so"
    assert "orbx_rigbow.h" in build.HEADERS
    rec = [l for l in build.LIBS if l.out == build.RIGBOW_OUT]
    assert len(rec) == 1 and rec[0].sources == (build.RIGBOW_SOURCE,) and rec[0].hidden and not rec[0].product


def test_rigbow_library_exports_exactly_its_header():
    from orb_slam3_modified_amd import _lib, build
    build.build()
    names = _declared("orbx_rigbow.h")
    assert len(names) == 6 and all(n.startswith("orbx_rigbow_") for n in names), names
    exported = _exported(_lib.RIGBOW_LIB_PATH)
    assert {e for e in exported if e.startswith("orbx_")} == set(names)
    assert not [e for e in exported if not e.startswith("orbx_rigbow_") and not e.startswith("_")], sorted(exported)[:10]   # -fvisibility=hidden


def test_the_other_libraries_keep_their_exports():
    from orb_slam3_modified_amd import _lib, build
    build.build()
    rnames = set(_declared("orbx_rigbow.h"))
    assert not rnames & _exported(_lib.LIB_PATH) and not rnames & set(_declared("orbx.h"))
    assert not rnames & _exported(_lib.MATCH_LIB_PATH)
    assert {e for e in _exported(_lib.MATCH_LIB_PATH) if e.startswith("orbx_")} == set(_declared("orbx_match.h")) and len(_declared("orbx_match.h")) == 5
    assert {e for e in _exported(_lib.LIB_PATH) if e.startswith("orbx_")} >= set(_declared("orbx.h"))
    assert len(_declared("orbx.h")) <= 100
    assert build.kernels_hash() == KERNELS_HASH
    assert os.path.dirname(build.RIGBOW_SOURCE) == "rigbow" and "orbx_rigbow.hip" not in os.listdir(build.CSRC)


def test_python_binding_covers_the_header():
    from orb_slam3_modified_amd import _lib, build
    build.build()
    M = _lib.rigbow_lib()
    assert set(M._orbx_rigbow_symbols) == set(_declared("orbx_rigbow.h"))
    from orb_slam3_modified_amd import rigbow
    assert issubclass(rigbow.RigBowBatch, _lib.SideHandle)
    for m in ("stack_device", "bow_pairs", "bow_pairs_device"):
        assert callable(getattr(rigbow.RigBowBatch, m))
    # the structures the binding passes are the header's
    for struct, cls, size in (("orbx_rigbow_side", _lib.OrbxRigBowSide, 9 * 8 + 2 * 4), ("orbx_rigbow_rig", _lib.OrbxRigBowRig, 6 * 8 + 3 * 4 + 4)):
        in_header = abi_util.struct_fields("orbx_rigbow.h", struct)
        assert in_header == [f for f, _ in cls._fields_], in_header
        assert C.sizeof(cls) == size
    # orbx_match_side's fields, then d_nleft before the sizes
    assert [f for f, _ in _lib.OrbxRigBowSide._fields_] == [f for f, _ in _lib.OrbxMatchSide._fields_][:8] + ["d_nleft", "nframes", "capacity"]
    assert (rigbow.FRAME, rigbow.KEYFRAMES) == (0, 1) and rigbow.lds_bytes(3000, 3000) <= rigbow.LDS_MAX < 36 * 6000 + 16 * 3000 + 4 * 3000


def test_bad_arguments_are_rejected_without_a_device():
    """Argument checks that come before any device call."""
    from orb_slam3_modified_amd import _lib
    M = _lib.rigbow_lib()
    h = C.c_void_p(0)
    assert M.orbx_rigbow_create(None, 0) == _lib.ORBX_E_INVALID
    assert b"null" in M.orbx_rigbow_last_error(None)
    assert M.orbx_rigbow_create(C.byref(h), -1) == _lib.ORBX_E_INVALID and not h.value
    assert b"device" in M.orbx_rigbow_last_error(None)
    side, rig = _lib.OrbxRigBowSide(), _lib.OrbxRigBowRig()
    assert M.orbx_rigbow_pairs_device(None, C.byref(side), C.byref(side), None, 1, 0, 0.7, 1, None, None, None, None) == _lib.ORBX_E_INVALID
    assert M.orbx_rigbow_pairs_device(None, None, None, None, 0, 7, 0.7, 1, None, None, None, None) == _lib.ORBX_E_INVALID
    assert M.orbx_rigbow_pairs(None, None, None, None, 1, 0, 0.7, 1, None, None, None) == _lib.ORBX_E_INVALID
    assert M.orbx_rigbow_stack_device(None, C.byref(rig), 8, None, None, None, None, None) == _lib.ORBX_E_INVALID
    M.orbx_rigbow_destroy(None)


@abi_util.needs_hipcc
def test_rigbow_kernels_compile_without_scratch():
    from orb_slam3_modified_amd.build import RIGBOW_SOURCE
    scratch = abi_util.kernel_scratch(RIGBOW_SOURCE, hidden=True)
    assert len([n for n in scratch if "k_rigbow_pairs" in n]) == 2 and len([n for n in scratch if "k_rigbow_stack" in n]) == 1, sorted(scratch)
    assert len(scratch) == 3 and all(v == 0 for v in scratch.values()), scratch
