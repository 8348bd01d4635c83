"""tests/rigbow_model.py, the sequential statement of the rig SearchByBoW and of the stacked rig frame (include/orbx_rigbow.h): held to
the claims of the constructed batch (tests/rigbow_cases.py) on its own trace, and to the single-camera model (tests/match_batch_model.py)
where the two must agree (CPU only)."""
import numpy as np
import pytest

from tests import match_batch_cases as mc
from tests import match_batch_model as mm
from tests import rigbow_cases as rc
from tests import rigbow_model as rm

F32 = np.float32
COMBOS = [(mode, valid, ori) for mode in (rm.FRAME, rm.KEYFRAMES) for valid in (True, False) for ori in (True, False)]


def model_pair(c, ia, ib, mode, ratio, valid, ori, trace=None):
    (da, aa, va, fa, nla), (db, ab, vb, fb, nlb) = rc.frame(c, ia), rc.frame(c, ib)
    return rm.search_by_bow(da, aa, va if valid else None, fa, nla, db, ab, vb if valid else None, fb, nlb, mode, ratio, ori, trace=trace)


@pytest.fixture(scope="module")
def case():
    """The batch and -- computed once -- the model's (nmatches, b2a, a2b) and trace of every planted pair under every run, mode, valid form
    and check_orientation."""
    c = rc.build()
    for run, ratio in rc.RUNS.items():
        for mode, valid, ori in COMBOS:
            for p, (ia, ib) in enumerate(rc.PAIRS.tolist()):
                tr = []
                c["want", run, mode, valid, ori, p] = model_pair(c, ia, ib, mode, ratio, valid, ori, tr)
                c["trace", run, mode, valid, ori, p] = tr
    return c


def _query(c, key, name):
    """The trace entry of the planted query `name`, or None when it did not run."""
    hit = [t for t in c[("trace",) + key + (rc.CLAIMS[name][0],)] if t.get("a") == rc.PLANTED[name]]
    assert len(hit) <= 1
    return hit[0] if hit else None


def test_the_planted_nodes_hold_what_they_claim(case):
    c = case
    assert len(rc.PAIRS) <= 8 and len(rc.BAD_PAIRS) <= 8 and rc.CAP <= 256
    for name, (p, run, want) in rc.CLAIMS.items():
        for mode, valid, ori in COMBOS:
            wl, wr = want(mode, valid, ori)
            a2b = c["want", run, mode, valid, ori, p][2]
            held = tuple(int(v) for v in a2b[rc.PLANTED[name]])
            assert held == (-1 if wl is None else rc.KP[wl], -1 if wr is None else rc.KP[wr]), (name, mode, valid, ori, held)
    # whole-result invariants: b2a and a2b say the same, the column is the slot's camera, keyframes mode binds one slot a query
    for key, (n, b2a, a2b) in ((k, v) for k, v in c.items() if k[0] == "want"):
        _, run, mode, valid, ori, p = key
        nlb = int(c["nleft"][rc.PAIRS[p, 1]])
        assert n == (b2a >= 0).sum() == (a2b >= 0).sum()
        for slot in np.nonzero(b2a >= 0)[0]:
            col = int(mode == rm.FRAME and nlb != -1 and slot >= nlb)
            assert a2b[b2a[slot], col] == slot
        if mode == rm.KEYFRAMES:
            assert (a2b[:, 1] == -1).all()


def test_each_site_is_the_edge_it_names(case):
    """Read off the trace: the distances a site rests on are the ones the query saw."""
    c = case
    fr = ("main", rm.FRAME, False, False)
    kf = ("main", rm.KEYFRAMES, False, False)
    t = _query(c, fr, "l50")
    assert (t["best1"], t["best2"], t["best1r"]) == (50, 256, 10) and t["left"] >= 0 and t["right"] >= 0
    assert _query(c, kf, "l50")["left"] == -1                              # < 50 between keyframes
    t = _query(c, fr, "l51_r0")
    assert (t["best1"], t["best1r"], t["left"], t["right"]) == (51, 0, -1, -1)
    t = _query(c, fr, "ratio_fails_right_binds")
    assert (t["best1"], t["best2"], t["best1r"]) == (rc.BEST, rc.SECOND, 20) and t["left"] == -1 and t["right"] == rc.KP["ratio_fails_right_binds:r0"]
    assert _query(c, fr, "r50")["best1r"] == 50 and _query(c, fr, "r50")["right"] >= 0
    assert _query(c, fr, "r51")["best1r"] == 51 and _query(c, fr, "r51")["right"] == -1 and _query(c, fr, "r51")["left"] >= 0
    t = _query(c, fr, "r_tie")
    assert t["best1r"] == t["best2r"] == 20 and t["right"] == rc.KP["r_tie:r1"] > rc.KP["r_tie:r0"]   # first in list order, not by index
    lst = c["fv"][rc.B0][t["node"]]
    assert lst.index(rc.KP["r_tie:r1"]) < lst.index(rc.KP["r_tie:r0"])
    nlb = int(c["nleft"][rc.B0])
    for name in ("all_right", "no_left_candidate_left"):
        t = _query(c, fr, name)
        assert all(i >= nlb for i in c["fv"][rc.B0][t["node"]]) and t["best1"] == 256 and t["best1r"] <= 3 and (t["left"], t["right"]) == (-1, -1)
    t = _query(c, fr, "right_listed_first")
    lst = c["fv"][rc.B0][t["node"]]
    assert lst[0] >= nlb > lst[1] and (t["left"], t["right"]) == (lst[1], lst[0])
    t1, t2 = _query(c, fr, "taken_first"), _query(c, fr, "taken_second")
    assert t1["skipped"] == [] and sorted(t2["skipped"]) == sorted([t1["left"], t1["right"]]) and t1["left"] < nlb <= t1["right"]
    assert (t2["left"], t2["right"]) == (rc.KP["taken:l1"], rc.KP["taken:r1"])
    t = _query(c, fr, "second_ignores_right")
    assert (t["best1"], t["best2"], t["best1r"]) == (30, 200, 31) and not F32(30) < F32(rc.RATIO) * F32(31) and t["left"] >= 0
    # a right-camera keyframe feature is a query towards a frame and none between keyframes
    assert rc.PLANTED["right_query"] >= c["nleft"][rc.A0] and _query(c, fr, "right_query")["left"] >= 0 and _query(c, kf, "right_query") is None
    assert _query(c, ("main", rm.FRAME, True, False), "invalid_a") is None and _query(c, fr, "invalid_a") is not None
    # two histogram entries of one query in different bins, one of which loses
    key = ("main", rm.FRAME, False, True)
    t = _query(c, key, "rot_two_bins")
    end = c[("trace",) + key + (rc.P_ROT,)][-1]
    assert t["left"] >= 0 and t["right"] >= 0 and end["removed"] == [t["right"]] and end["bins"][0] == 13 and end["bins"][3] == 1
    a, l, r = c["kps"][rc.A2]["angle"][t["a"]], c["kps"][rc.B2]["angle"][t["left"]], c["kps"][rc.B2]["angle"][t["right"]]
    assert (mm.rotation_bin(a, l), mm.rotation_bin(a, r)) == (0, 3)
    # nleft = 0: every B feature is right, nothing is bound in either mode; = count and = -1: the single-camera result
    assert (c["nleft"][rc.B3], c["nleft"][rc.B5]) == (0, -1) and c["nleft"][rc.B4] == c["counts"][rc.B4, 0]
    for mode in (rm.FRAME, rm.KEYFRAMES):
        assert c["want", "main", mode, False, True, rc.P_NL0][0] == 0
        n1, b1, a1 = c["want", "main", mode, False, True, rc.P_NLCOUNT]
        n2, b2, a2 = c["want", "main", mode, False, True, rc.P_SINGLE]
        assert n1 == n2 == 3 and np.array_equal(b1, b2) and np.array_equal(a1, a2)
    assert c["nleft"][rc.B5] == -1 and c["want", "main", rm.FRAME, False, True, rc.P_SINGLE_A][0] >= 2


def test_the_big_nodes(case):
    """65 and 72 candidates take two trips, 64 stay in registers; the twice-standing minima sit on different trips."""
    c = case
    sizes = {name: len(c["fv"][rc.B1][n]) for name, n in (("nb_65", 165), ("nb_64", 164), ("nb_72", 172))}
    assert sizes == rc.N_BIG
    nlb = int(c["nleft"][rc.B1])
    for n in (165, 164, 172):
        lst = c["fv"][rc.B1][n]
        cams = [i >= nlb for i in lst]
        assert any(cams[j] != cams[j + 1] for j in range(len(lst) - 1))           # the cameras interleave along the list
        assert [i for i in lst if i < nlb] == sorted([i for i in lst if i < nlb], reverse=True)
    lst = c["fv"][rc.B1][165]
    for lo, hi in ((10, 64), (11, 63)):
        assert lst[lo] == rc.KP["nb_65:%d" % lo] and lst[hi] == rc.KP["nb_65:%d" % hi]
    assert 10 // 64 != 64 // 64 and 64 % 64 < 10 % 64
    lst = c["fv"][rc.B1][172]
    assert lst[7] == rc.KP["nb_72:7"] and lst[71] == rc.KP["nb_72:71"] and 7 % 64 == 71 % 64 and 6 % 64 == 70 % 64
    t = [x for x in c["trace", "main", rm.FRAME, False, False, rc.P_BIG] if x.get("node") == 172][0]
    assert (t["best1"], t["best2"], t["best1r"], t["best2r"]) == (20, 22, 20, 20) and t["left"] == -1 and t["right"] == rc.KP["nb_72:7"]
    t = [x for x in c["trace", "high", rm.FRAME, False, False, rc.P_BIG] if x.get("node") == 165]
    assert len(t) == 2 and t[0]["best1"] == t[0]["best2"] == 20 and sorted(t[1]["skipped"]) == sorted([t[0]["left"], t[0]["right"]])


def test_the_float32_facts_the_sites_rest_on():
    best, second, ratio = rc.BEST, rc.SECOND, rc.RATIO
    assert F32(ratio) * F32(second) == F32(best) and not F32(best) < F32(ratio) * F32(second) and best <= 50
    assert float(best) < float(F32(ratio)) * second                             # in double the test would pass
    assert F32(0.7) * F32(50) == F32(35) and not F32(35) < F32(0.7) * F32(50) and F32(34) < F32(0.7) * F32(50)
    assert F32(50) < F32(ratio) * F32(256) and F32(30) < F32(ratio) * F32(200) and F32(20) < F32(ratio) * F32(40)
    assert not F32(20) < F32(ratio) * F32(22) and not F32(20) < F32(ratio) * F32(20) and F32(20) < F32(1.5) * F32(20)
    assert F32(0.1) * F32(13) > F32(1) and mm.three_maxima([13, 0, 0, 1] + [0] * 26) == [0, -1, -1]
    assert mm.rotation_bin(100.0, 100.0) == 0 and mm.rotation_bin(100.0, 10.0) == 3


def test_each_malformed_kind(case):
    c = case
    assert sorted(rc.MALFORMED.values()) == sorted(["frame", "negative count", "negative fv_n", "fv_feat entry at its frame's count",
                                                    "nleft below -1", "nleft above the count"])
    for p, (ia, ib) in enumerate(rc.BAD_PAIRS.tolist()):
        args = []
        for f in (ia, ib):
            ok = 0 <= f < rc.K
            g = f if ok else 0
            k = max(int(c["fv_n"][g]), 0)
            args += [int(c["counts"][g, 0]), int(c["fv_n"][g]), c["fv_feat"][g, :c["fv_ptr"][g, k]].tolist(), int(c["nleft"][g]), ok]
        bad = rm.malformed(*(args[0:4] + [args[4]] + args[5:9] + [args[9]]))
        assert bad == (p in rc.MALFORMED), (p, args)
    assert c["counts"][rc.NEGCOUNT, 0] < 0 and c["fv_n"][rc.NEGFV] < 0 and c["nleft"][rc.NLLOW] == -2
    assert c["nleft"][rc.NLHIGH] == c["counts"][rc.NLHIGH, 0] + 1
    f = rc.BADFEAT
    assert (c["fv_feat"][f, :c["fv_ptr"][f, c["fv_n"][f]]] >= c["counts"][f, 0]).sum() == 1
    for f in range(rc.K):                                                    # the arrays say what the dicts say
        if f not in (rc.BADFEAT, rc.NEGFV):
            got = {int(c["fv_node"][f, j]): c["fv_feat"][f, c["fv_ptr"][f, j]:c["fv_ptr"][f, j + 1]].tolist() for j in range(int(c["fv_n"][f]))}
            assert got == c["fv"][f] and list(got) == sorted(got), f


@pytest.mark.parametrize("mode", [rm.FRAME, rm.KEYFRAMES])
def test_single_camera_frames_give_the_single_camera_model(mode):
    """With every nleft = -1 the model is tests/match_batch_model.py on tests/match_batch_cases.py's batch."""
    c = mc.build()
    done = 0
    for run, ratio in mc.RUNS.items():
        for valid in (True, False):
            for ori in (True, False):
                for p, (ia, ib) in enumerate(mc.PAIRS.tolist()):
                    if p in mc.MALFORMED:
                        continue
                    (da, aa, va, fa), (db, ab, vb, fb) = mc.frame(c, ia), mc.frame(c, ib)
                    va, vb = (va, vb) if valid else (None, None)
                    wn, wb2a = mm.search_by_bow(da, aa, va, fa, db, ab, vb, fb, mode, ratio, ori)
                    n, b2a, a2b = rm.search_by_bow(da, aa, va, fa, -1, db, ab, vb, fb, -1, mode, ratio, ori)
                    assert n == wn and np.array_equal(b2a, wb2a) and np.array_equal(a2b[:, 0], mm.invert(wb2a, len(da))) and (a2b[:, 1] == -1).all()
                    done += 1
    assert done == len(mc.RUNS) * 4 * (len(mc.PAIRS) - len(mc.MALFORMED))


def test_keyframes_mode_is_the_single_camera_model_on_the_left_features(case):
    """:800 and :820 are `valid &= idx < nleft` on both sides."""
    c = case
    total = 0
    for run, ratio in rc.RUNS.items():
        for valid in (True, False):
            for p, (ia, ib) in enumerate(rc.PAIRS.tolist()):
                (da, aa, va, fa, nla), (db, ab, vb, fb, nlb) = rc.frame(c, ia), rc.frame(c, ib)
                va = (va if valid else np.ones(len(da), np.uint8)) & (np.arange(len(da)) < (nla if nla != -1 else len(da)))
                vb = (vb if valid else np.ones(len(db), np.uint8)) & (np.arange(len(db)) < (nlb if nlb != -1 else len(db)))
                wn, wb2a = mm.search_by_bow(da, aa, va, fa, db, ab, vb, fb, mm.KEYFRAMES, ratio, True)
                n, b2a, a2b = c["want", run, rm.KEYFRAMES, valid, True, p]
                assert n == wn and np.array_equal(b2a, wb2a) and np.array_equal(a2b[:, 0], mm.invert(wb2a, len(da)))
                total += n
    assert total > 20


def test_the_stacker_model():
    kl, dl, cl, kr, dr, cr = rc.rig_frames()
    ks, ds, cs, nleft = rm.stack(kl, dl, cl, kr, dr, cr, rc.CAP_S)
    for f, (nl, nr) in enumerate(rc.RIG_COUNTS):
        if f in rc.RIG_MALFORMED:
            assert cs[f].tolist() == [-1, 0] and nleft[f] == -1 and not ds[f].any() and not ks[f].tobytes().strip(b"\0")
            continue
        assert cs[f].tolist() == [nl + nr, 0] and nleft[f] == nl
        assert np.array_equal(ds[f, :nl], dl[f, :nl]) and np.array_equal(ds[f, nl:nl + nr], dr[f, :nr]) and not ds[f, nl + nr:].any()
        assert ks[f, :nl].tobytes() == kl[f, :nl].tobytes() and ks[f, nl:nl + nr].tobytes() == kr[f, :nr].tobytes()
    assert sorted(rc.RIG_MALFORMED.values()) == sorted(["nl + nr above cap_s", "negative left count", "right count above cap_r", "left count above cap_l"])
    assert rc.RIG_COUNTS[2] == (rc.CAP_L, rc.CAP_S - rc.CAP_L) and rc.RIG_COUNTS[3][0] + rc.RIG_COUNTS[3][1] == rc.CAP_S + 1
    assert rc.RIG_COUNTS[5][1] == rc.CAP_R + 1 and rc.RIG_COUNTS[6][0] == rc.CAP_L + 1 and rc.CAP_L % 4 == 0 and rc.RIG_COUNTS[0][0] % 4 != 0
