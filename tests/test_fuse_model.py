"""tests/fuse_model.py, the specification of the batched Fuse search, held pair by pair to oracle.pyoracle.window_nearest (CPU only)."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import fuse_cases as fc
from tests import fuse_model as fm


@pytest.fixture(scope="module")
def case():
    c = fc.build()
    inv = fc.inv_level_sigma2()
    c["inv"] = inv
    for gate in (False, True):
        st = {}
        c["want", gate] = fm.search(c["kps"], c["desc"], c["counts"], c["uright"], c["gridparm"], c["query"], c["nquery"], c["pairs"], c["pdesc"],
                                    inv, gate, 50, stats=st)
        c["stats", gate] = st
    return c


def _oracle_row(c, p, gate, kps=None, desc=None, uright=None, parm=None):
    k = int(c["pairs"][p])
    n = int(c["counts"][k, 0])
    sel = fc.finite_queries(c, p)
    q = c["query"][p, sel]
    parm = c["gridparm"][k]
    grid = dict(min_x=parm[0], min_y=parm[1], inv_w=parm[2], inv_h=parm[3])
    extra = dict(kp_uright=c["uright"][k, :n], inv_level_sigma2=c["inv"], q_ur=q["ur"]) if gate else {}
    return sel, po.window_nearest(c["kps"][k, :n], c["desc"][k, :n], grid, q["x"], q["y"], q["r"], q["min_level"], q["max_level"],
                                  c["pdesc"][q["point"]], **extra)


@pytest.mark.parametrize("gate", (False, True))
def test_the_model_is_the_oracle_on_the_constructed_cases(case, gate):
    c = case
    nfound, bidx, bdist = c["want", gate]
    assert (c["query"]["max_level"][c["query"]["point"] >= 0] >= 0).all()       # where the oracle's level convention is the reference loop's
    for p in range(len(c["pairs"])):
        sel, (oi, od) = _oracle_row(c, p, gate)
        assert np.array_equal(bidx[p, sel], oi) and np.array_equal(bdist[p, sel], od), (gate, p)
        rest = np.setdiff1d(np.arange(fc.QCAP), sel)
        assert (bidx[p, rest] == -1).all() and (bdist[p, rest] == 256).all()
        assert nfound[p] == (od <= 50).sum()


def test_the_planted_cases_are_what_they_claim(case):
    c = case
    (n0, bi0, bd0), (n1, bi1, bd1) = c["want", False], c["want", True]
    at = lambda name, a: int(a[fc.PLANTED[name]])   # noqa: E731
    assert at("dup_one_cell", bi0) == 7 and at("dup_one_cell", bd0) == 0                 # ascending index inside a cell
    assert at("dup_two_columns", bi0) == 140 and at("dup_two_columns", bd0) == 0         # walk order, not index order
    assert at("edge_out", bi0) != 33 and at("edge_in", bi0) == 33 and at("edge_in", bd0) == 0   # |distx| == r is out
    assert at("gate_stereo", bi0) == 90 and at("gate_stereo", bi1) == -1                 # 1 * float32(7.8) > 7.8 in double
    assert at("gate_mono", bi0) == 91 and at("gate_mono", bi1) == 91                     # 1 * float32(5.99) < 5.99 in double
    assert np.float32(1.0) * np.float32(7.8) <= np.float32(7.8)                          # a float32 comparison would keep the stereo one
    for name in ("return_min_x", "return_max_x", "return_min_y", "return_max_y", "skipped"):
        assert at(name, bi0) == -1 and at(name, bd0) == 256, name
    assert at("clip_left", bd0) <= 256 and at("wide", bi0) >= 0
    nq = int(c["nquery"].sum())
    found0, found1 = int((bi0 >= 0).sum()), int((bi1 >= 0).sum())
    assert found1 < found0 and 3 * found1 >= nq, (found0, found1, nq)                    # the gate bites; a third of all queries still find
    assert c["stats", False].get("ties", 0) > 0 and c["stats", True].get("gated", 0) > 0
    assert sorted(set(c["nquery"].tolist()) & {0, 1, 63, 64, 65, fc.QUERIES_PER_WORKGROUP + 1}) == [0, 1, 63, 64, 65, fc.QUERIES_PER_WORKGROUP + 1]
    assert np.bincount(c["pairs"], minlength=fc.K)[fc.FULL] >= 2 and c["counts"][fc.FULL, 0] == fc.CAP and c["counts"][fc.EMPTY, 0] == 0
    cells = fm.assign_grid(c["kps"][fc.ONE_CELL, :100], c["gridparm"][fc.ONE_CELL])
    assert [len(x) for x in cells if x] == [100]


def test_the_grid_is_the_oracles(case):
    c = case
    for k in range(fc.K):
        n = int(c["counts"][k, 0])
        start, order = po.assign_grid(c["kps"][k, :n], *c["gridparm"][k])
        cells = fm.assign_grid(c["kps"][k, :n], c["gridparm"][k])
        assert [i for cell in cells for i in cell] == order.tolist()
        assert np.array_equal(np.cumsum([0] + [len(cell) for cell in cells]), start)


def test_malformed_pairs_in_the_model(case):
    c = case
    q = c["query"].copy()
    q[1, 3]["point"] = len(c["pdesc"])
    pairs = c["pairs"].copy()
    pairs[2], pairs[4] = fc.K, -1
    nquery = c["nquery"].copy()
    nquery[5] = fc.QCAP + 1
    nf, bi, bd = fm.search(c["kps"], c["desc"], c["counts"], c["uright"], c["gridparm"], q[:6], nquery[:6], pairs[:6], c["pdesc"], c["inv"], False)
    assert nf[[1, 2, 4, 5]].tolist() == [-1] * 4 and (bi[[1, 2, 4, 5]] == -1).all() and (bd[[1, 2, 4, 5]] == 256).all()
    assert nf[0] == c["want", False][0][0] and np.array_equal(bi[3], c["want", False][1][3])


def test_the_model_is_the_oracle_on_extracted_keypoints():
    """Two frames of the golden extraction as keyframes, each searched with queries derived from the other, with and without the gate."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "extractor_small.npz"))
    fk, fd = [g["g320_0_kps"], g["g320_1_kps"]], [g["g320_0_desc"], g["g320_1_desc"]]
    cap = 304
    kps, desc, counts = np.zeros((2, cap), fk[0].dtype), np.zeros((2, cap, 32), np.uint8), np.zeros((2, 2), np.int32)
    uright = np.full((2, cap), -1.0, np.float32)
    for f in range(2):
        n = len(fk[f])
        kps[f, :n], desc[f, :n], counts[f, 0] = fk[f], fd[f], n
        uright[f, :n] = np.where(np.arange(n) % 2 == 0, fk[f]["x"] - np.float32(5.0), np.float32(-1.0))
    parm = np.stack([fc.grid_parameters(0, 0, 320, 240)] * 2)
    pdesc = np.concatenate(fd)
    rows = [fc.derived_queries(fk[1], cap, 5, len(fk[0])), fc.derived_queries(fk[0], cap, 6, 0)]
    query, nquery = np.stack([r for r, _ in rows]), np.array([n for _, n in rows], np.int32)
    inv = fc.plain_inv_level_sigma2()
    found = {}
    for gate in (False, True):
        nf, bi, bd = fm.search(kps, desc, counts, uright, parm, query, nquery, np.array([0, 1], np.int32), pdesc, inv, gate)
        for p in range(2):
            n = counts[p, 0]
            sel = np.nonzero(query[p]["point"] >= 0)[0]
            q = query[p, sel]
            extra = dict(kp_uright=uright[p, :n], inv_level_sigma2=inv, q_ur=q["ur"]) if gate else {}
            oi, od = po.window_nearest(kps[p, :n], desc[p, :n], dict(min_x=parm[p, 0], min_y=parm[p, 1], inv_w=parm[p, 2], inv_h=parm[p, 3]),
                                       q["x"], q["y"], q["r"], q["min_level"], q["max_level"], pdesc[q["point"]], **extra)
            assert np.array_equal(bi[p, sel], oi) and np.array_equal(bd[p, sel], od), (gate, p)
        found[gate] = int((bi >= 0).sum())
    assert found[True] < found[False] and found[True] > 100, found
