"""tests/stereo_model.py (a numpy restatement of Frame::ComputeStereoMatches, src/Frame.cc:811-981) held to the oracle, and the constructed
batch of tests/stereo_cases.py held to its claims: every planted keypoint took the branch it was planted for, every counter of the model
fired, the domain holds.  Pyramids here are the oracle extractor's.  No GPU."""
import numpy as np
import pytest

from oracle import pyoracle as po
from orb_slam3_modified_amd import synth
from tests import stereo_cases as sc
from tests import stereo_model as sm

F32 = np.float32


def _pyramids(ex, img):
    ex.extract(img)
    return [ex.level(l) for l in range(sc.NLEVELS)]


@pytest.fixture(scope="module")
def case():
    """The batch, the oracle's pyramids of every frame and -- computed once -- the model's result of every frame under every run."""
    c = sc.build()
    ex = po.OracleExtractor(*sc.PARAMS)
    c["pyrL"] = [_pyramids(ex, c["L"][f]) for f in range(sc.NF)]
    c["pyrR"] = [_pyramids(ex, c["R"][f]) for f in range(sc.NF)]
    c["tables"] = ex.tables()
    for run, (mb, mbf) in sc.RUNS.items():
        for f in range(sc.NF):
            c["model", run, f] = sm.compute_stereo_matches(*sc.frame(c, f), c["pyrL"][f], c["pyrR"][f], sc.SCALE, sc.INV, mb, mbf)
    return c


@pytest.mark.parametrize("run", list(sc.RUNS))
def test_the_model_is_the_oracle_on_the_constructed_batch(case, run):
    c = case
    mb, mbf = sc.RUNS[run]
    for f in range(sc.NF):
        ou, od, ok = po.stereo_matches(*sc.frame(c, f), c["pyrL"][f], c["pyrR"][f], sc.SCALE, sc.INV, mb, mbf)
        u, d, k, _ = c["model", run, f]
        assert k == ok and u.tobytes() == ou.tobytes() and d.tobytes() == od.tobytes(), (run, f)


def test_the_model_is_the_oracle_on_extracted_frames():
    L, R, _ = synth.make_stereo_pairs(2, sc.H, sc.W, seed=13, noise=2)
    ex = po.OracleExtractor(*sc.PARAMS)
    for f in range(2):
        kL, dL, _ = ex.extract(L[f])
        pl = [ex.level(l) for l in range(sc.NLEVELS)]
        kR, dR, _ = ex.extract(R[f])
        pr = [ex.level(l) for l in range(sc.NLEVELS)]
        for mb, mbf in sc.RUNS.values():
            ou, od, ok = po.stereo_matches(kL, dL, kR, dR, pl, pr, sc.SCALE, sc.INV, mb, mbf)
            u, d, k, st = sm.compute_stereo_matches(kL, dL, kR, dR, pl, pr, sc.SCALE, sc.INV, mb, mbf)
            assert k == ok and u.tobytes() == ou.tobytes() and d.tobytes() == od.tobytes(), f
            assert len(kL) > 100 and len(kR) > 100 and st["border"] == st["delta"] == st["maxu_negative"] == 0
        assert ok > 20                                            # the EuRoC run: the pair's disparities fit


def test_the_domain_and_the_tables(case):
    c = case
    sc.assert_domain(c)
    t = c["tables"]
    assert t["scale"].tobytes() == sc.SCALE.tobytes() and t["inv_scale"].tobytes() == sc.INV.tobytes()
    assert [p.shape for p in c["pyrL"][0]] == sc.SIZES and np.array_equal(c["pyrL"][sc.A][0], c["L"][sc.A])
    assert sum(max(int(q) + 3, 32) for q in t["quota"]) == sc.CAP           # the product's capacity rule (4 * 8 root nodes or quota + 3 per level)
    assert F32(sc.RUNS["exact"][1]) / F32(sc.RUNS["exact"][0]) == 40 and F32(sc.RUNS["euroc"][1]) / F32(sc.RUNS["euroc"][0]) > sc.W
    assert (c["L"][:, sc.FLAT0:] == sc.G).sum() > 0.95 * c["L"][:, sc.FLAT0:].size and c["L"][:, :sc.FLAT0].std() > 20
    assert np.array_equal(c["L"][sc.A, :sc.FLAT0], c["R"][sc.A, :sc.FLAT0])


@pytest.mark.parametrize("run", list(sc.RUNS))
def test_every_planted_keypoint_took_its_branch(case, run):
    c = case
    res = {f: c["model", run, f][:3] for f in range(sc.NF)}
    sc.check_outcomes(c, run, res)
    for name, cl in sc.CLAIMS.items():
        if run != "exact" and cl["euroc"] is None:
            continue
        branches, u, _ = sc.expect(cl, run)
        st = c["model", run, cl["frame"]][3]
        assert st["branch"][cl["iL"]] in branches, (name, run, st["branch"][cl["iL"]], st["rec"][cl["iL"]])
        if cl["best"] is not None and run == "exact":
            assert st["rec"][cl["iL"]]["best_idx"] == cl["best"], (name, st["rec"][cl["iL"]])
    if run == "exact":
        rec = lambda name: c["model", run, sc.CLAIMS[name]["frame"]][3]["rec"][sc.CLAIMS[name]["iL"]]   # noqa: E731
        assert rec("ham_74")["best_dist"] == 74 and rec("ham_75")["best_dist"] == 75 and rec("ham_99")["best_dist"] == 99
        assert rec("ham_100")["best_dist"] == 100 and rec("ham_100")["passed"] == 1 and rec("ham_100")["best_idx"] == -1
        assert rec("sad_symmetric")["delta"] == 0 and rec("sad_symmetric")["sads"][6] == rec("sad_symmetric")["sads"][8]
        assert rec("sad_asymmetric")["delta"] == sc.CLAIMS["sad_asymmetric"]["delta"] != 0
        assert [rec(n)["inc"] for n in ("shift_m5", "shift_m4", "shift_p4", "shift_p5")] == [-5, -4, 4, 5]
        s = rec("sad_equal_shifts")["sads"]
        assert s[5] == s[8] == min(s) == 11 and rec("sad_equal_shifts")["inc"] == 0
        assert rec("disp_zero")["disparity"] == 0 and rec("disp_40")["disparity"] == 40 and rec("disp_39")["disparity"] == 39
        assert rec("disp_negative")["disparity"] == -2
        for n, lvl in (("border_nearest_l0", 0), ("border_nearest_l7", 7)):
            assert rec(n)["endu"] == sc.SIZES[lvl][1] - 6               # the largest endu of the domain: one more column is not reachable
        for f, sads in ((sc.M2, [10, 30]), (sc.M4, [10, 10, 10, 50]), (sc.M3_21, [10, 10, 21]), (sc.MZERO, [0, 0, 0])):
            assert c["model", run, f][3]["filter"]["sads"] == sads
        assert "filter" not in c["model", run, sc.M0][3] and c["model", run, sc.M1][3]["filter"]["n"] == 1


def test_every_counter_of_the_model_fired(case):
    c = case
    total = {k: sum(int(c["model", "exact", f][3][k]) for f in range(sc.NF)) for k in sm.COUNTERS}
    assert [k for k, v in total.items() if v == 0] == list(sc.UNREACHABLE), total
    seen = {b for f in range(sc.NF) for b in c["model", "exact", f][3]["branch"]}
    assert seen == set(sm.BRANCHES) - set(sc.UNREACHABLE)


def test_the_layout_the_sites_rest_on(case):
    """Right indices of the ties (lanes, trips, tiles), the four shared left slots and their gates, the tails and the count frames."""
    c = case
    for name, (lo, hi) in sc.TIES.items():
        cl = sc.CLAIMS[name]
        kL, dL, kR, dR = sc.frame(c, cl["frame"])
        assert sorted(cl["rights"]) == [lo, hi] and cl["best"] == lo
        assert sm._hamming(dL[cl["iL"]], dR[lo]) == sm._hamming(dL[cl["iL"]], dR[hi]) == 30 and kR[lo]["x"] != kR[hi]["x"]
    (lo, hi) = sc.TIES["tie_trip"]
    assert lo % 64 == hi % 64 and lo // 64 != hi // 64
    (lo, hi) = sc.TIES["tie_lanes"]
    assert hi == lo + 1 and lo // 64 == hi // 64 and all(lo // t == hi // t for t in sc.TILES)
    assert all(sc.TIES["tie_tile%d" % t][1] % t == 0 and sc.TIES["tie_tile%d" % t][0] == sc.TIES["tie_tile%d" % t][1] - 1 for t in sc.TILES)
    # the shared trip: slots 4w .. 4w + 3 = a, c, b, d; k0 passes a's gates only, k1 a's and c's, k2 those of a, c and b; d's none
    sh = sc.SHARE
    kL, dL, kR, dR = sc.frame(c, sh["frame"])
    assert sh["first"] % 4 == 0 and [sc.CLAIMS["share_" + s]["iL"] - sh["first"] for s in "acbd"] == [0, 1, 2, 3]

    def passes(iR):
        out = []
        for k in range(4):
            kp, r = kL[sh["first"] + k], kR[iR]
            minr, maxr = sm.row_band(r["y"], int(r["octave"]), sc.SCALE)
            out.append(bool(minr <= int(kp["y"]) <= maxr and abs(int(r["octave"]) - int(kp["octave"])) <= 1 and kp["x"] - F32(40) <= r["x"] <= kp["x"]))
        return out
    assert passes(sh["k0"]) == [True, False, False, False] and passes(sh["k1"]) == [True, True, False, False]
    assert passes(sh["k2"]) == [True, True, True, False]
    b = sc.CLAIMS["share_b"]["iL"]
    assert sm._hamming(dL[b], dR[sh["k1"]]) < sm._hamming(dL[b], dR[sh["k2"]]) < 75          # a leaked k1 would win slot b, and leave its gate
    # the tails
    tail = sc.CLAIMS["tail_live"]
    n = int(c["countsL"][tail["frame"], 0])
    assert tail["iL"] == n - 1 and n % 4 == 1 and n % 16 != 0
    assert c["countsL"][sc.FULL, 0] == sc.CAP and sc.CLAIMS["full_last"]["iL"] == sc.CAP - 1
    # the count frames: their keypoints would match
    assert c["countsR"][sc.NR0, 0] == 0 and c["countsR"][sc.NR1, 0] == 1 and c["countsR"][sc.RNEG, 0] == -1 and c["countsL"][sc.LNEG, 0] == -1
    ex_mb, ex_mbf = sc.RUNS["exact"]
    for f in (sc.NR0, sc.RNEG, sc.LNEG):
        nL, nR = int(c["nL"][f]), int(c["nR"][f])
        _, _, k, _ = sm.compute_stereo_matches(c["kpsL"][f, :nL], c["descL"][f, :nL], c["kpsR"][f, :nR], c["descR"][f, :nR], c["pyrL"][f], c["pyrR"][f],
                                               sc.SCALE, sc.INV, ex_mb, ex_mbf)
        assert k == 3 and c["model", "exact", f][2] == 0
    assert 0 < min(sc.RNEG, sc.LNEG) and max(sc.RNEG, sc.LNEG) < sc.NF - 1 and abs(sc.RNEG - sc.LNEG) > 1   # each has a neighbour on both sides


def test_the_float32_facts_the_sites_rest_on():
    k = F32(1.5) * F32(1.4)
    assert k * F32(10) == F32(21) and float(k) * 10 < 21            # the product rounds up to 21: SAD 21 is not below it, in float or in double
    assert F32(20) < k * F32(10) and not F32(21) < k * F32(10)
    assert F32(30) < k * F32(30) and not F32(30) < k * F32(10)      # (10, 30): the upper median keeps both, the lower one would not
    assert not F32(0) < k * F32(0)
    u = F32(100)
    assert F32(float(u) - 0.01) == F32(99.99) and F32(40) / F32(0.01) == F32(4000)   # the 0.01 branch at uL = 100: u_right 99.99f, depth 4000
    assert F32(60) >= u - F32(40) and not np.nextafter(F32(60), F32(-np.inf)) >= u - F32(40)
    assert sm._round(2.5) == 3 and sm._round(0.5) == 1 and sm.row_band(F32(158.0), 0, sc.SCALE) == (156, 160)
    assert sm.row_band(F32(0.5), 1, sc.SCALE)[0] == -2 and sm.row_band(F32(0.0), 7, sc.SCALE)[0] < -1
