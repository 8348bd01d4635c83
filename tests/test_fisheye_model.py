"""tests/fisheye_model.py and tests/fisheye_cases.py hold what the GPU suite of the batched two-camera rig front-end assumes of them: the
model's tables are the oracle's 2-NN of the lapping rows, its ratio test is the reference's float / double expression over every pair of
distances, and the constructed batch exercises every planted case (CPU only)."""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import fisheye_cases as fc
from tests import fisheye_model as fm

RATIO_C = r"""
/* src/Frame.cc:1151 with DMatch::distance's type */
static int lowe(int d0, int d1) { float a = (float)d0, b = (float)d1; return a < b * 0.7; }
void table(unsigned char* out) { for (int i = 0; i <= 256; i++) for (int j = 0; j <= 256; j++) out[i * 257 + j] = (unsigned char)lowe(i, j); }
"""


@pytest.fixture(scope="module")
def case():
    c = fc.build()
    c["match"] = fm.match(c["descL"], c["countsL"], c["descR"], c["countsR"])
    return c


def _brute(q, t):
    """The two smallest (distance, index) of every query by a full sort."""
    d = np.unpackbits(q[:, None, :] ^ t[None, :, :], axis=2).sum(2).astype(np.int64)
    order = np.argsort(d * 4096 + np.arange(len(t))[None, :], axis=1)[:, :2]
    return order, np.take_along_axis(d, order, 1)


def test_model_tables_are_the_oracles_knn2_of_the_lapping_rows(case):
    knn_idx, knn_dist, pairs, npairs = case["match"]
    for f, name in enumerate(fc.NAMES):
        (nL, mL), (nR, mR) = fc.FRAMES[name]
        if name in fc.EMPTY or name in fc.MALFORMED:
            assert npairs[f] == (-1 if name in fc.EMPTY else -2), name
            assert (knn_idx[f] == -1).all() and (knn_dist[f] == 256).all() and (pairs[f]["left"] == -1).all(), name
            continue
        outside = np.ones(fc.CAP_L, bool)
        outside[mL:nL] = False
        assert (knn_idx[f, outside] == -1).all() and (knn_dist[f, outside] == 256).all(), name
        idx, dist = po.knn2(case["descL"][f, mL:nL], case["descR"][f, mR:nR])
        if nL > mL:
            want = np.where(idx >= 0, idx + mR, -1)
            assert np.array_equal(knn_idx[f, mL:nL], want) and np.array_equal(knn_dist[f, mL:nL], dist), name
        if nL > mL and nR - mR >= 2:
            bi, bd = _brute(case["descL"][f, mL:nL], case["descR"][f, mR:nR])
            assert np.array_equal(knn_idx[f, mL:nL], bi + mR) and np.array_equal(knn_dist[f, mL:nL], bd), name
        # the pairs: ascending left rows, each the accepted head of its row, {-1, -1} behind them
        n = int(npairs[f])
        p = pairs[f, :n]
        assert (np.diff(p["left"]) > 0).all() and (pairs[f, n:]["left"] == -1).all() and (pairs[f, n:]["right"] == -1).all()
        ok = (knn_idx[f, :, 1] >= 0) & fm.ratio_accept(knn_dist[f, :, 0], knn_dist[f, :, 1])
        assert np.array_equal(p["left"], np.nonzero(ok)[0]) and np.array_equal(p["right"], knn_idx[f, ok, 0]), name
    counts = dict(zip(fc.NAMES, npairs.tolist()))
    assert counts["q1_t1"] == 0 and counts["q0_left_mono_is_n"] == 0 and counts["t0_right_mono_is_n"] == 0
    assert counts["main"] > 64 and min(counts[n] for n in ("q63_t2_mono0", "q64_t63", "q65_t64", "q30_t65")) > 8
    f = fc.NAMES.index("q1_t1")
    assert knn_idx[f, 199].tolist() == [99, -1] and knn_dist[f, 199, 1] == 256 and knn_dist[f, 199, 0] < 256
    f = fc.NAMES.index("t0_right_mono_is_n")
    assert (knn_idx[f] == -1).all()


def test_ratio_expression_over_all_pairs_of_distances(tmp_path):
    d0, d1 = np.meshgrid(np.arange(257), np.arange(257), indexing="ij")
    got = fm.ratio_accept(d0, d1)
    # numpy with explicit types, one operation at a time
    a, b = d0.astype(np.float32), d1.astype(np.float32)
    prod = np.multiply(b.astype(np.float64), np.float64(0.7), dtype=np.float64)
    assert np.array_equal(got, np.less(a.astype(np.float64), prod))
    # on these integers the rounded product never crosses the comparison: the integer form agrees everywhere (70 < 100 * 0.7 is false,
    # as 100 * 0.7 rounds to 70.0) -- the library evaluates the reference's expression all the same
    assert np.array_equal(got, 10 * d0 < 7 * d1)
    assert not got[7, 10] and not got[14, 20] and not got[21, 30] and got[69, 99] and not got[70, 100] and not got[0, 0] and got[0, 1]
    if shutil.which("gcc"):                                              # the reference's own expression, compiled
        src, lib = tmp_path / "ratio.c", tmp_path / "ratio.so"
        src.write_text(RATIO_C)
        subprocess.check_call(["gcc", "-O0", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(lib), str(src)])
        out = np.zeros((257, 257), np.uint8)
        C.CDLL(str(lib)).table(out.ctypes.data_as(C.c_void_p))
        assert np.array_equal(out.astype(bool), got)


def test_planted_expectations(case):
    knn_idx, knn_dist, pairs, npairs = case["match"]
    P = fc.PLANTED
    main = fc.NAMES.index("main")
    accepted = set(pairs[main, :npairs[main]]["left"].tolist())
    for d0, d1 in fc.RATIO_EDGE:
        assert "ratio_%d_%d" % (d0, d1) in P
    for name, v in P.items():
        if "dist" not in v:
            continue
        f, q = v["frame"], v["left"]
        assert tuple(knn_idx[f, q]) == tuple(v["right"]) and tuple(knn_dist[f, q]) == v["dist"], name
        assert v["right"][0] < v["right"][1] or v["dist"][0] < v["dist"][1], name
        assert (q in accepted) == (10 * v["dist"][0] < 7 * v["dist"][1]), name
    for name in ("ratio_7_10", "ratio_14_20", "ratio_21_30", "ratio_70_100", "ratio_0_0", "ratio_8_10", "ratio_15_20", "ratio_22_30", "ratio_70_99",
                 "ratio_71_100", "duplicate_train_rows", "duplicate_across_the_tile_boundary"):
        assert P[name]["left"] not in accepted, name
    for name in ("ratio_6_10", "ratio_13_20", "ratio_20_30", "ratio_69_99", "ratio_68_99", "ratio_69_100", "ratio_0_1", "identical_to_a_train_row"):
        assert P[name]["left"] in accepted, name
    # ties: equal distances, the lower train row first; the pair either side of the small tile's first boundary
    for name in ("duplicate_train_rows", "duplicate_across_the_tile_boundary"):
        (a, b), (d0, d1) = P[name]["right"], P[name]["dist"]
        assert a < b and d0 == d1
    a, b = P["duplicate_across_the_tile_boundary"]["right"]
    mR = fc.FRAMES["main"][1][1]
    assert (a - mR) // fc.SMALL_TILE == 0 and (b - mR) // fc.SMALL_TILE == 1 and b == a + 1
    assert knn_dist[main, P["identical_to_a_train_row"]["left"], 0] == 0
    # rows outside the ranges are never named
    for name in ("monocular_row_is_ignored", "row_past_the_count_is_ignored"):
        v = P[name]
        assert v["never"] not in knn_idx[v["frame"], v["left"]].tolist() and knn_dist[v["frame"], v["left"], 0] > 0, name
    # the train counts at the small tile's edges, the query counts at a wave's
    trains = {fc.FRAMES[n][1][0] - fc.FRAMES[n][1][1] for n in fc.NAMES if n not in fc.EMPTY + fc.MALFORMED}
    queries = {fc.FRAMES[n][0][0] - fc.FRAMES[n][0][1] for n in fc.NAMES if n not in fc.EMPTY + fc.MALFORMED}
    assert {0, 1, 2, fc.SMALL_TILE - 1, fc.SMALL_TILE, fc.SMALL_TILE + 1} <= trains and {0, 1, 63, 64, 65} <= queries
    assert 8 <= fc.B <= 12 and max(fc.CAP_L, fc.CAP_R) <= 320


def test_finish_collisions_and_depth_edges(case):
    knn_idx, knn_dist, pairs, npairs = case["match"]
    P = fc.PLANTED
    main = fc.NAMES.index("main")
    depth_in = fc.pair_depths(pairs, npairs)
    l2r, r2l, depth, nmatches = fm.finish(pairs, npairs, depth_in, case["countsL"], case["countsR"], fc.CAP_R)
    for name in ("collision_last_rejected", "collision_last_accepted"):
        v = P[name]
        assert [int(knn_idx[main, q, 0]) for q in v["lefts"]] == [v["right"]] * 3, name
        assert np.nonzero(pairs[main, :npairs[main]]["right"] == v["right"])[0].size == 3, name
    a, b = P["collision_last_rejected"], P["collision_last_accepted"]
    assert r2l[main, a["right"]] == a["lefts"][1] and l2r[main, a["lefts"][2]] == -1 and l2r[main, a["lefts"][0]] == a["right"]
    assert r2l[main, b["right"]] == b["lefts"][2] and l2r[main, b["lefts"][1]] == -1 and l2r[main, b["lefts"][0]] == b["right"]
    for name, carrier in fc.DEPTH_CARRIERS.items():
        q = P[carrier]["left"]
        value, taken = fc.DEPTH_EDGE[name]
        k = int(np.nonzero(pairs[main, :npairs[main]]["left"] == q)[0][0])
        assert depth_in[main, k].tobytes() == value.tobytes(), name
        assert (l2r[main, q] >= 0) == taken and (depth[main, q].tobytes() == value.tobytes()) == taken, name
    assert fc.DEPTH_EDGE["depth_next_above"][0] > np.float32(0.0001) and np.isnan(fc.DEPTH_EDGE["depth_nan"][0])
    # a status is handed on; a well-formed frame counts its accepted depths
    for f, name in enumerate(fc.NAMES):
        if npairs[f] < 0:
            assert nmatches[f] == npairs[f] and (l2r[f] == -1).all() and (r2l[f] == -1).all() and (depth[f] == -1).all(), name
        else:
            assert nmatches[f] == (l2r[f] >= 0).sum() == (depth[f] > 0).sum() and 0 <= nmatches[f] <= npairs[f], name
    assert 0 < nmatches[main] < npairs[main]
    # malformed pairs: outside the counts, or not ascending
    bad = pairs.copy()
    bad[main, 3]["left"] = fc.CAP_L
    assert fm.finish(bad, npairs, depth_in, case["countsL"], case["countsR"], fc.CAP_R)[3][main] == -2
    bad = pairs.copy()
    bad[main, [4, 5]] = bad[main, [5, 4]]
    assert fm.finish(bad, npairs, depth_in, case["countsL"], case["countsR"], fc.CAP_R)[3][main] == -2


def test_the_rig_frames_meet_their_floor_on_the_oracle_alone():
    """What tests/test_gpu_fisheye.py's device-resident chain asserts of its inputs holds on the CPU: nonempty lapping ranges on both sides
    and at least RIG_MIN_PAIRS accepted pairs a frame."""
    from tests import trimatch_cases as tc
    left, right = fc.rig_frames()
    ox = po.OracleExtractor(*tc.EXTRACTOR)
    cap = tc.EXTRACTOR[0] + 3 * tc.EXTRACTOR[2]
    L = [ox.extract(left[f], fc.RIG_LAP_L) for f in range(fc.RIG_FRAMES)]
    R = [ox.extract(right[f], fc.RIG_LAP_R) for f in range(fc.RIG_FRAMES)]
    cL = np.array([(len(k), m) for k, _, m in L], np.int32)
    cR = np.array([(len(k), m) for k, _, m in R], np.int32)
    assert (cL[:, 1] < cL[:, 0]).all() and (cR[:, 1] < cR[:, 0]).all() and (cL[:, 1] > 0).all() and (cR[:, 1] > 0).all()
    npairs = fm.match(fc.padded([d for _, d, _ in L], cap, np.uint8, 32), cL, fc.padded([d for _, d, _ in R], cap, np.uint8, 32), cR)[3]
    assert npairs.tolist() == [118, 111, 114, 110] and npairs.min() >= fc.RIG_MIN_PAIRS
