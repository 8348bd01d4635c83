"""csrc/side/orbx_window_device.h and orbx_window_host.h: the one statement of the frame grid, the window and the chain the four chained
projection matchers share (liborbx_localmatch.so, liborbx_lastmatch.so, liborbx_projmatch.so, liborbx_rigmatch.so).  CPU-only checks."""
import os
import re
import shutil
import subprocess

import pytest

from tests import abi_util
from tests import rigmatch_cases as rc

ROOT = abi_util.ROOT
SIDE = os.path.join(ROOT, "orb_slam3_modified_amd", "csrc", "side")
SHAPES = ((1, 1), (72, 64), (1024, 2048), (5024, 1024), (32768, 1))
RIG_SHAPES = ((1, 1, 1), (rc.CAP_L, rc.CAP_R, rc.MCAP), (1024, 1024, 2048), (1500, 1500, 2000), (16384, 16384, 1))


@pytest.fixture(scope="module")
def window_check(tmp_path_factory):
    """tests/support/window_check.cpp, built with the host compiler from the header's plain-C++ part and run once."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("window") / "window_check")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "support", "window_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    return r.stdout


def test_div_rn_is_the_float_division_bit_for_bit(window_check):
    m = re.search(r"div_rn: (\d+) comparisons, (\d+) mismatches", window_check)
    assert m and int(m.group(2)) == 0 and "MISMATCH" not in window_check, window_check[-2000:]
    assert int(m.group(1)) > 2 * (4 * (1 << 23) + 2000000)     # both dividends: the significand sweeps and the random divisors


def test_the_bindings_sizing_formula_is_the_headers_layout(window_check):
    from orb_slam3_modified_amd import _window
    got = {(int(c), int(q)): int(v) for c, q, v in re.findall(r"^layout (\d+) (\d+) (\d+)$", window_check, flags=re.M)}
    assert set(got) == set(SHAPES)
    for cap, mcap in SHAPES:
        assert _window.lds_bytes(cap, mcap) == got[cap, mcap], (cap, mcap)
    assert int(re.search(r"^lds_max (\d+)$", window_check, flags=re.M).group(1)) == _window.LDS_MAX


def test_the_room_the_gpu_test_states_is_the_layouts(window_check):
    """rigmatch.lds_bytes() is rig_layout(...).fixed of the header, run on the host, for the GPU test's shape, larger ones and the edges."""
    from orb_slam3_modified_amd import build, rigmatch, _window
    got = {(int(a), int(b), int(q)): int(v) for a, b, q, v in re.findall(r"^rig_layout (\d+) (\d+) (\d+) (\d+)$", window_check, flags=re.M)}
    assert set(got) == set(RIG_SHAPES) and {(1, 1, 1), (16384, 16384, 1), (rc.CAP_L, rc.CAP_R, rc.MCAP)} <= set(got)
    for shape in RIG_SHAPES:
        assert rigmatch.lds_bytes(*shape) == got[shape], shape
    assert rigmatch.lds_bytes is rigmatch.RigMatchBatch.lds_bytes is _window.rig_lds_bytes and "def lds_bytes" not in open(rigmatch.__file__).read()
    total = got[rc.CAP_L, rc.CAP_R, rc.MCAP]
    # plan_paths (csrc/side/orbx_handle.h) on the three limits the GPU test creates its handles with: the LDS path with room for
    # SMALL_ROOM candidates under the lowered limit, more than every item's lists under the default one, the global path under 0
    handle = open(os.path.join(build.CSRC, "side", "orbx_handle.h")).read()
    assert "p->in_lds = fixed_lds + 4 * (size_t)longest <= limit;" in handle and "(int)((limit - fixed_lds) / 4)" in handle

    def plan(lds_limit):
        limit = lds_limit & ~15
        return (limit - total) // 4 if total + 4 * rc.SLOTS <= limit else None   # the room on the LDS path, None: the global path
    assert plan(total + 4 * rc.SMALL_ROOM) == rc.SMALL_ROOM and plan(0) is None and plan(rigmatch.LDS_MAX) > 8 * rc.SMALL_ROOM


def test_the_grid_and_the_window_are_stated_once():
    from orb_slam3_modified_amd import build, lastmatch, localmatch, projmatch, rigmatch, _window
    core = open(os.path.join(SIDE, "orbx_window_device.h")).read()
    host = open(os.path.join(SIDE, "orbx_window_host.h")).read()
    for name in ("float div_rn(", "Lay layout(", "void build_grid(", "void walk(", "void scan_offsets(", "int chunk_end(", "int rotation_filter(",
                 "struct Bump {", "GridLay grid_layout(", "struct RigLay {", "RigLay rig_layout(", "Arrays arrays(", "int open_top(", "int open_second(", "struct LaneKeys {", "int ratio_test(",
                 "void bind(", "void publish(", "void last_writer(", "constexpr int kThHigh", "__hip_atomic_fetch_max(", '__builtin_amdgcn_fence('):
        assert core.count(name) == 1 and name not in host, name
    assert core.count("wave_min(") == 2 and core.count("auto add = ") == 0          # open_top's and open_second's reductions; one bump allocator
    for name in ("side_problem(const S* s)", "int check_call(", "int sort_size(", "plan_paths(", "int launch(", "wait_previous(", "record_call(",
                 "struct StagedSide {", "StagedSide stage_side(", "S device_side("):
        assert host.count(name) == 1 and name not in core, name
    assert host.count("hipLaunchKernelGGL(") == 2                                   # the LDS and the global instantiation, once
    bitonic = re.compile(r"for \(int k = 2; k <= \w+; k <<= 1\)")
    three_maxima = re.compile(r"for \(int i = 0; i < kBins; i\+\+\)")
    assert len(bitonic.findall(core)) == 1 and len(three_maxima.findall(core)) == 1
    for source in (build.LOCALMATCH_SOURCE, build.LASTMATCH_SOURCE, build.PROJMATCH_SOURCE, build.RIGMATCH_SOURCE):
        src = open(os.path.join(build.CSRC, source)).read()
        assert '#include "../side/orbx_window_device.h"' in src and '#include "../side/orbx_window_host.h"' in src, source
        for own in ("div_rn(float", "Lay layout(", "struct Lay", "side_problem(const", "void walk(", "plan_paths(", "ComputeThreeMaxima,",
                    "__hip_atomic_fetch_max", "wave_min(", "struct RigLay", "rig_chunk_end", "rig_layout(int", "auto add = ", "__builtin_amdgcn_fence",
                    "hipLaunchKernelGGL", "wait_previous(", "record_call(", "kThHigh =", "p2 <<= 1", "p2l <<= 1", "s_hist", "d_kps, nk"):
            assert own not in src, (source, own)
        assert not three_maxima.search(src) and "kBins" not in src, source
        assert src.count("launch(m, path, g, ") == 1 and ("stage_side(io, side" in src), source
        assert not bitonic.search(src) and not re.search(r"constexpr int k(Threads|LdsMax|MaxBlocks|GlobalBlocks|GlobalRoom|Cols|None)\b", src), source
        lib = [l for l in build.LIBS if l.sources == (source,)]
        assert len(lib) == 1 and set(build.WINDOW_CORE) <= set(lib[0].deps), source
    for f in build.WINDOW_CORE:
        assert os.path.dirname(f) == "side" and os.path.isfile(os.path.join(build.CSRC, f))      # below csrc/: outside kernels_hash()
    for name in ("lds_bytes", "_table", "_up16"):
        assert getattr(localmatch, name) is getattr(lastmatch, name) is getattr(projmatch, name) is getattr(_window, name), name
    assert rigmatch._table is _window._table
    assert localmatch.LDS_MAX == lastmatch.LDS_MAX == projmatch.LDS_MAX == rigmatch.LDS_MAX == _window.LDS_MAX
    assert "kLdsMax = %d * 1024" % (_window.LDS_MAX // 1024) in core
    for mod in (localmatch, lastmatch, projmatch, rigmatch):
        text = open(mod.__file__).read()
        assert "def lds_bytes" not in text and "def _table" not in text and "def _up16" not in text, mod.__name__
