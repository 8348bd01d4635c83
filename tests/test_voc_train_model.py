"""Vocabulary training without a GPU: the glibc rand() restatement, the numpy model of create against the reference's goldens, the golden
maker, and the zero-scratch rule for the training library's kernels."""
import ctypes
import hashlib
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import abi_util, voc_train_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "voc_train.npz")
GOLDEN_SHA256 = "592b0e1ac844aed818e2f4858636c09493677e772991a64faf882f5640d44f26"   # written by tools/make_voc_train_golden.py
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


@abi_util.needs_hipcc
def test_training_kernels_use_no_scratch():
    """The rule of tests/test_kernel_resources.py for the training library's translation unit (that test walks build.SOURCES only)."""
    from orb_slam3_modified_amd.build import TRAIN_SOURCE
    scratch = abi_util.kernel_scratch(TRAIN_SOURCE)   # one size per kernel, or it raises
    assert len(scratch) >= 8
    assert not any(scratch.values()), scratch
