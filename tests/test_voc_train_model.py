"""Vocabulary training without a GPU: the glibc rand() restatement, the numpy model of create against the reference's goldens, the golden
maker, the zero-scratch rule for the training library's kernels, and the large-node cases (tests/voc_train_cases.py): their generators, the
model against the reference's recorded trees, and the guard that every case reaches the regime of csrc/train/orbx_train.hip it is named for."""
import ctypes
import hashlib
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import abi_util, voc_train_cases as VC, voc_train_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "voc_train.npz")
GOLDEN_SHA256 = "592b0e1ac844aed818e2f4858636c09493677e772991a64faf882f5640d44f26"   # written by tools/make_voc_train_golden.py
LARGE = os.path.join(ROOT, "tests", "golden", "voc_train_large.npz")
LARGE_SHA256 = "2bcefc607456cb7481eb85cef16645e734e7dadffdf476b4d99a1e35e6588e82"    # written by tools/make_voc_train_golden.py --large
SEEDS = (0, 1, 7, 12345, 2 ** 31 + 5, 2 ** 32 - 1)


def _libc_rand(seed, n):
    libc = ctypes.CDLL("libc.so.6")
    libc.srand(ctypes.c_uint(seed))
    return np.array([libc.rand() for _ in range(n)], np.int32)


@pytest.mark.parametrize("seed", SEEDS)
def test_library_rand_equals_libc_rand(seed):
    """liborbx_train.so draws from its own restatement of glibc's srand / rand (the caller's random state stays untouched)."""
    from orb_slam3_modified_amd._lib import train_lib
    n = 10 ** 6
    out = np.zeros(n, np.int32)
    assert train_lib().orbx_train_glibc_rand(seed, n, out.ctypes.data) == 0
    assert np.array_equal(out, _libc_rand(seed, n))


@pytest.mark.parametrize("seed", SEEDS)
def test_model_rand_equals_libc_rand(seed):
    r = M.GlibcRand(seed)
    assert np.array_equal(np.array([r.next() for _ in range(20000)], np.int32), _libc_rand(seed, 20000))


def test_golden_file_is_the_committed_one():
    assert hashlib.sha256(open(GOLDEN, "rb").read()).hexdigest() == GOLDEN_SHA256


def test_golden_covers_what_create_must_reproduce():
    z = np.load(GOLDEN)
    cfg = {str(n): tuple(int(x) for x in z[f"cfg_{n}"]) for n in z["configs"]}
    assert {c[0] for c in cfg.values()} >= {2, 5, 10, 16}
    assert {c[1] for c in cfg.values()} >= {1, 2, 3, 4}
    assert {c[2] for c in cfg.values()} == {0, 1, 2, 3}
    assert len({c[4] for c in cfg.values()}) >= 2
    assert any(str(z[f"cfg_{n}_set"]) == "few" for n in cfg)       # fewer distinct descriptors than k
    assert any(str(z[f"cfg_{n}_set"]) == "tiny" for n in cfg)      # n <= k at the root
    assert os.path.getsize(GOLDEN) < 1 << 20


@pytest.mark.parametrize("name", [str(n) for n in np.load(GOLDEN)["configs"]])
def test_model_equals_reference_create(name):
    z = np.load(GOLDEN)
    k, L, w, s, seed = (int(x) for x in z[f"cfg_{name}"])
    dset = str(z[f"cfg_{name}_set"])
    got, _ = M.create(z[f"in_{dset}_desc"], z[f"in_{dset}_off"], k, L, w, seed)
    for key, a in zip(("parent", "leaf", "desc", "weight"), got):
        assert np.array_equal(a, z[f"out_{name}_{key}"]), (name, key)


def test_model_departures():
    """An empty cluster keeps its centre (the reference crashes there); too few iterations raise instead of looping."""
    z = np.load(GOLDEN)
    (parent, leaf, d, w), st = M.create(z["in_clustered_desc"], z["in_clustered_off"], 10, 3, 0, 7)
    assert st["empty_clusters"] > 0 and len(parent) > 10
    with pytest.raises(M.NoConvergence):
        M.create(z["in_synth_desc"], z["in_synth_off"], 10, 2, 0, 1, max_iterations=1)


@pytest.mark.skipif(not os.path.isdir(os.environ.get("REFROOT", "/root/reference")) or shutil.which("g++") is None,
                    reason="the reference tree is not on this machine")
def test_golden_maker_reproduces_the_committed_golden():
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_voc_train_golden.py"), "--check"], cwd=ROOT)


# ---- the large-node cases -------------------------------------------------------------------------------------------------------------
_large = {}


def large(name):
    """(desc, offsets, the model's tree, its stats, its trace) of one case, computed once for all tests below and never changed."""
    if name not in _large:
        c = VC.CASES[name]
        desc, off = VC.generate(name)
        trace = []
        tree, st = M.create(desc, off, c["k"], c["L"], c["weighting"], c["seed"], trace=trace)
        desc.flags.writeable = False
        _large[name] = (desc, off, tree, st, trace)
    return _large[name]


def test_large_golden_file_is_the_committed_one():
    assert hashlib.sha256(open(LARGE, "rb").read()).hexdigest() == LARGE_SHA256
    assert os.path.getsize(LARGE) < 1 << 20
    z = np.load(LARGE)
    assert [str(n) for n in z["cases"]] == list(VC.CASES)
    assert not any(f.startswith("in_") for f in z.files)          # outputs and settings only
    for name, c in VC.CASES.items():
        assert [int(x) for x in z[f"cfg_{name}"]] == [c["k"], c["L"], c["weighting"], c["scoring"], c["seed"], c["mid"]]
        assert str(z[f"gen_{name}"]) == c["gen"] and np.array_equal(z[f"args_{name}"], np.array(c["args"], np.float64))
        assert np.array_equal(z[f"off_{name}"], c["offsets"])


@pytest.mark.parametrize("name", list(VC.CASES))
def test_large_generators_reproduce_the_recorded_inputs(name):
    desc, off = large(name)[:2]
    assert desc.shape == (VC.CASES[name]["args"][0], 32) and desc.dtype == np.uint8
    assert VC.digest(desc, off) == str(np.load(LARGE)[f"sha_{name}"])


@pytest.mark.parametrize("name", list(VC.CASES))
def test_model_equals_reference_create_on_large_nodes(name):
    z = np.load(LARGE)
    _, _, tree, st, trace = large(name)
    for key, a in zip(("parent", "leaf", "desc", "weight"), tree):
        assert np.array_equal(a, z[f"out_{name}_{key}"]), (name, key)
    c = VC.CASES[name]
    assert [st["empty_clusters"], st["iterations"]] == z[f"model_{name}_stats"].tolist()
    assert st["empty_clusters"] == 0                               # the reference completes on none with an empty cluster
    want = [(thr,) + VC.split(trace, c["k"], thr) for thr in (c["k"] + 1, c["mid"], VC.DEFAULT_MIN_NODE, VC.HOST_ONLY)]
    assert z[f"model_{name}_split"].tolist() == [list(r) for r in want]


def test_trace_changes_nothing():
    z = np.load(GOLDEN)
    args = (z["in_clustered_desc"], z["in_clustered_off"], 5, 2, 1, 8)
    trace = []
    a, sa = M.create(*args)
    b, sb = M.create(*args, trace=trace)
    assert sa == sb and all(np.array_equal(x, y) for x, y in zip(a, b))
    assert trace[0]["level"] == 1 and trace[0]["n"] == 3000 and len(trace[0]["draws"]) == trace[0]["kc"] - 1 == 4
    for n, s, cut, idx in trace[0]["draws"]:
        assert n == 3000 and 0 < cut <= s and 0 <= idx < n


def _root_picks(name):
    root = large(name)[4][0]
    assert root["level"] == 1 and root["n"] == VC.CASES[name]["args"][0]
    return root, [idx for _, _, _, idx in root["draws"]]


def test_guard_edges_picks_sit_on_block_edges_on_both_sides_of_the_chunk_boundary():
    """Every pick of k_seed_select at the root is a block's first or last element, in the first chunk of 256 blocks and in the carried one,
    and the seeding stops early (sum == 0) with one centre per distinct descriptor."""
    c = VC.CASES["edges_66k"]
    root, picks = _root_picks("edges_66k")
    others = c["args"][1]
    assert root["first"] % VC.BLOCK not in (0, VC.BLOCK - 1)       # the first centre is A
    assert all(p % VC.BLOCK in (0, VC.BLOCK - 1) for p in picks)
    assert {p % VC.BLOCK for p in picks} == {0, VC.BLOCK - 1}
    assert min(picks) < VC.CHUNK <= max(picks)
    assert root["kc"] == others + 1 < c["k"]
    # the children are all duplicates: one centre each, on a node above k
    kids = [t for t in large("edges_66k")[4] if t["level"] == 2]
    assert len(kids) == others + 1 and all(t["kc"] == 1 and t["n"] > c["k"] and not t["draws"] for t in kids)
    assert max(t["n"] for t in kids) > VC.CHUNK - VC.BLOCK * 2     # the duplicates of A: 256 blocks on the device


def test_guard_chunks_and_stride_picks_cross_the_chunks():
    _, picks = _root_picks("chunks_70k")
    assert min(picks) < VC.CHUNK <= max(picks)
    assert -(-VC.CASES["chunks_70k"]["args"][0] // VC.BLOCK) == 274
    _, picks = _root_picks("stride_262k")
    assert len({p // VC.CHUNK for p in picks}) >= 3
    n = VC.CASES["stride_262k"]["args"][0]
    nb = -(-n // VC.BLOCK)
    assert nb == 1024 + 2 and n % VC.BLOCK == 77                    # k_bitcount: workgroup 0 takes a full second tile, workgroup 1 one of 77 rows


@pytest.mark.parametrize("name,product,per,busy", [("scan_1024", 1024, 1, 1024), ("scan_1040", 1040, 2, 520)])
def test_guard_scan_products(name, product, per, busy):
    """k_scan_excl at the root: m = kc * nb entries, per = ceil(m / 1024) a thread, `busy` threads with a non-empty range."""
    c = VC.CASES[name]
    root, _ = _root_picks(name)
    nb = -(-root["n"] // VC.BLOCK)
    assert root["kc"] == c["k"] == 16 and root["kc"] * nb == product
    assert -(-product // 1024) == per and -(-product // per) == busy
    assert any(t["level"] == 2 and t["n"] > c["k"] for t in large(name)[4])
    if name == "scan_1040":
        assert root["n"] % VC.BLOCK == 1                            # a one-row last block


@pytest.mark.parametrize("name", VC.IDF_CASES)
def test_guard_idf_documents(name):
    """5 to 9 uneven documents with one empty one, no boundary on a multiple of 256 or 65536; the empty document counts in NDocs; where N
    allows, some word's Ni counts a document that lies wholly past descriptor 65536."""
    desc, off, (parent, leaf, D, weight), _, _ = large(name)
    ndocs, lens = len(off) - 1, np.diff(off)
    assert 5 <= ndocs <= 9 and (lens == 0).sum() == 1 and len(set(lens.tolist())) == ndocs
    assert all(b % VC.BLOCK and b % VC.CHUNK for b in off[1:-1].tolist())
    word_of = M.descend(parent, leaf, D, desc)

    def ni(docs):
        out = {}
        for d in docs:
            for w in set(word_of[off[d]:off[d + 1]].tolist()):
                out[w] = out.get(w, 0) + 1
        return out

    full = ni(range(ndocs))
    for w, cnt in full.items():                                    # NDocs includes the empty document: every weight shows it
        assert weight[w] == np.log(float(ndocs) / float(cnt)) != np.log(float(ndocs - 1) / float(cnt))
    assert len({cnt for cnt in full.values()}) > 1                 # and the weights are not all one value
    past = [d for d in range(ndocs) if off[d] >= VC.CHUNK and lens[d] > 0]
    if len(desc) > VC.CHUNK:
        assert past
        assert ni(range(ndocs)) != ni([d for d in range(ndocs) if d not in past])
    # a descent that stopped after the first chunk would change a weight
    if len(desc) > VC.CHUNK:
        first = {}
        for d in range(ndocs):
            for w in set(word_of[off[d]:min(off[d + 1], VC.CHUNK)].tolist()) if off[d] < VC.CHUNK else ():
                first[w] = first.get(w, 0) + 1
        assert first != full


@pytest.mark.skipif(not os.path.isdir(os.environ.get("REFROOT", "/root/reference")) or shutil.which("g++") is None,
                    reason="the reference tree is not on this machine")
def test_golden_maker_reproduces_the_committed_large_golden():
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_voc_train_golden.py"), "--large", "--check"], cwd=ROOT)


@abi_util.needs_hipcc
def test_training_kernels_use_no_scratch():
    """The rule of tests/test_kernel_resources.py for the training library's translation unit (that test walks build.SOURCES only)."""
    from orb_slam3_modified_amd.build import TRAIN_SOURCE
    scratch = abi_util.kernel_scratch(TRAIN_SOURCE)   # one size per kernel, or it raises
    assert len(scratch) >= 8
    assert not any(scratch.values()), scratch
