"""tests/projmatch_model.py, the specification of the batched relocalization and Sim3 matchers, held point by point to the candidate lists
and distances of oracle.pyoracle.window_search_grid, and tests/projmatch_cases.py held to its claims on the model (CPU only)."""
import math

import numpy as np
import pytest

from tests import projmatch_cases as pc
from tests import projmatch_model as pm

F = np.float32
ORI = (True, False)


def run(c, ori, taken=True):
    return pm.search(c["kps"], c["desc"], c["counts"], c["bounds"], c["items"], c["points"], c["npts"], c["pdesc"], c["sf"], ori,
                     c["kp_taken"] if taken else None)


@pytest.fixture(scope="module")
def case():
    c = pc.build()
    for ori in ORI:
        c["want", ori] = run(c, ori)
    return c


def good_items(c):
    return [b for b in range(pc.B) if b not in pc.MALFORMED]


oracle_lists = pm.oracle_lists


def test_the_models_lists_are_the_oracles_and_taken_is_the_chains(case):
    """Every well-formed item: the candidates of every live point, in order, with their distances, equal window_search_grid's with
    (level - 1, level + 1) resp. (level - 1, level) and NO kp_skip: kp_taken is applied only in the chain (:504, :1952)."""
    c = case
    lists = total = hidden = 0
    for b in good_items(c):
        it, m = c["items"][b], int(c["npts"][b])
        f = int(it["frame"])
        n = int(c["counts"][f, 0])
        want = oracle_lists(c["kps"][f, :n], c["desc"][f, :n], c["bounds"][f], c["sf"], it, c["points"][b, :m], c["pdesc"])
        cells = pm.assign_grid(c["kps"][f, :n], c["bounds"][f])
        for q, w in want.items():
            got = pm.candidates(c["kps"][f, :n], c["desc"][f, :n], cells, c["bounds"][f], c["points"][b, q], c["pdesc"], c["sf"], it)
            assert got == w, (b, q)
            lists += 1
            total += len(w)
            hidden += sum(1 for i, _ in w if c["kp_taken"][b, i])
    assert lists > 500 and total > 3000 and hidden > 50           # taken keypoints stand in the lists
    # with the taken keypoints left out of the lists instead, the chain gives the same rows: the test is the chain's alone
    nm, match = c["want", True][:2]
    for b in (pc.I_RAND0, pc.I_RAND1, pc.I_PLANT0, pc.I_PLANT1):
        it, m = c["items"][b], int(c["npts"][b])
        f = int(it["frame"])
        n = int(c["counts"][f, 0])
        skipped = oracle_lists(c["kps"][f, :n], c["desc"][f, :n], c["bounds"][f], c["sf"], it, c["points"][b, :m], c["pdesc"], kp_skip=c["kp_taken"][b, :n])
        rows = [skipped.get(q) for q in range(m)]
        got = pm.chain(rows, c["points"][b], c["kps"][f], it, True, None, pc.CAP)
        assert got[0] == nm[b] and np.array_equal(got[1], match[b]), b
    # and without kp_taken the planted rows differ
    free = run(c, True, taken=False)
    assert not np.array_equal(free[1][pc.I_PLANT0], match[pc.I_PLANT0]) and not np.array_equal(free[1][pc.I_RAND1], match[pc.I_RAND1])


def test_the_planted_window_level_and_chain_cases_are_what_they_claim(case):
    c = case
    P, KP = pc.PLANTED, pc.KP
    nm, match, bound, _ = c["want", True]
    at = lambda name, b: int(bound[b, P[name]])   # noqa: E731
    # (a) the level edges: kind 0 takes level + 1 (at the top level - 1), kind 1 level - 1 (at the bottom the level itself); never +- 2
    for l, name in pc.LEVEL_SITES.items():
        want = {pc.RELOC: 1 if l + 1 < pc.NLEVELS else -1, pc.SIM3: -1 if l >= 1 else 0}
        for kind, b in pc.PLANT_ITEMS.items():
            assert c["items"][b]["kind"] == kind and at(name, b) == KP[name, want[kind]], (name, kind)
    assert at("lvl_mid", pc.I_PLANT0) != at("lvl_mid", pc.I_PLANT1)
    assert c["kps"][pc.PLANT, KP["lvl_mid", 1]]["octave"] == 4 and c["points"][pc.I_PLANT0, P["lvl_mid"]]["level"] == 3
    assert pm.level_range(pc.RELOC, 0) == (-1, 1) and pm.level_range(pc.SIM3, 0) == (-1, 0) and pm.level_range(pc.SIM3, 7) == (6, 7)
    assert sorted(pc.LEVEL_DIST.values()) == [0, 1, 5, 7, 10]      # a unique best under every range
    for kind, b in pc.PLANT_ITEMS.items():
        limit = c["items"][b]["max_dist"]
        # (b) the strict bound
        x = c["points"][b, P["bound_at"]]["u"]
        assert F(c["kps"][pc.PLANT, KP["bound_at"]]["x"] - x) == pm.radius_of(pc.TH, 0, c["sf"]) == F(3.0)
        x = c["points"][b, P["bound_inside"]]["u"]
        kx = c["kps"][pc.PLANT, KP["bound_inside"]]["x"]                                      # one ulp of the coordinate inside
        assert kx == np.nextafter(F(x + F(3.0)), F(0)) and F(kx - x) < F(3.0)
        assert at("bound_at", b) == -1 and at("bound_inside", b) == KP["bound_inside"]
        # (c) the accept limits
        for dist in (64, 65, 75, 76):
            pd = c["pdesc"][c["points"][b, P["dist", dist]]["point"]]
            assert pm.hamming(pd, c["desc"][pc.PLANT, KP["dist", dist]]) == dist
            assert at(("dist", dist), b) == (KP["dist", dist] if F(dist) <= limit else -1), (kind, dist)
        # (d) the tie
        assert at("tie", b) == KP["tie_first_column"] > KP["tie_later_column"]
        # (e) taken on entry
        assert c["kp_taken"][b, KP["entry_taken"]] and c["kp_taken"][b, KP["entry_only"]] and c["kp_taken"][b].sum() == 2
        assert at("entry", b) == KP["entry_free"] and at("entry_nothing", b) == -1
        assert match[b, KP["entry_taken"]] == -1 and match[b, KP["entry_only"]] == -1
        # (f) taken by an earlier point of the row
        assert at("first", b) == KP["wanted"] and at("falls_back", b) == KP["second_choice"] and P["first"] < P["falls_back"]
        assert at("first_alone", b) == KP["wanted_alone"] and at("falls_to_nothing", b) == -1
        # (g) the early returns, the non-finite projections, the invalid point
        for name in pc.RETURNS:
            assert at(name, b) == -1, name
        assert nm[b] == (bound[b] >= 0).sum() == (match[b] >= 0).sum()        # a keypoint is bound once
    assert LIMITS_ARE(c)
    # the limits of the two kinds: 64 / 65 fall on the two sides of 64.0, 75 / 76 on those of 50 * 1.5
    assert at(("dist", 64), pc.I_PLANT0) >= 0 and at(("dist", 65), pc.I_PLANT0) == -1
    assert at(("dist", 75), pc.I_PLANT1) >= 0 and at(("dist", 76), pc.I_PLANT1) == -1
    # a NaN limit accepts nothing, under both kinds
    for b in (pc.I_NAN0, pc.I_NAN1):
        assert math.isnan(c["items"][b]["max_dist"]) and nm[b] == 0 and (match[b] == -1).all()
        assert c["points"][b].tobytes() == c["points"][pc.I_PLANT0].tobytes()   # the same row (it holds a NaN)
    # the tie: two descriptors at the same distance, in two grid columns
    pd = c["pdesc"][c["points"][pc.I_PLANT0, P["tie"]]["point"]]
    da, db = c["desc"][pc.PLANT, KP["tie_first_column"]], c["desc"][pc.PLANT, KP["tie_later_column"]]
    assert pm.hamming(pd, da) == pm.hamming(pd, db) == 7 and not np.array_equal(da, db)
    col = lambda i: pm.cell_of(*c["kps"][pc.PLANT, i][["x", "y"]], c["bounds"][pc.PLANT]) // 48   # noqa: E731
    assert col(KP["tie_first_column"]) == 34 and col(KP["tie_later_column"]) == 35
    # the corner: (u - r) * inv_w reaches 64 exactly; each of the other four leaves by a return of its own
    p = c["points"][pc.I_PLANT0, P["return_corner"]]
    inv_w, inv_h = pm.grid_inverses(c["bounds"][pc.PLANT])
    assert math.floor(F(F(F(p["u"] - F(0)) - F(3.0)) * inv_w)) == 64
    r = F(3.0)
    cellx = lambda name, s: F(F(c["points"][pc.I_PLANT0, P[name]]["u"] + s * r) * inv_w)   # noqa: E731
    celly = lambda name, s: F(F(c["points"][pc.I_PLANT0, P[name]]["v"] + s * r) * inv_h)   # noqa: E731
    assert math.floor(cellx("return_min_x", -1)) >= 64 and math.ceil(cellx("return_max_x", 1)) < 0
    assert math.floor(celly("return_min_y", -1)) >= 48 and math.ceil(celly("return_max_y", 1)) < 0
    assert 0 <= math.floor(cellx("return_min_y", -1)) < 64 and 0 <= math.floor(cellx("return_max_y", -1)) < 64
    # (h) bounds with a non-zero origin: a keypoint at negative coordinates lies in a cell and is found
    assert c["bounds"][pc.RANDOM, 0] < 0 and c["bounds"][pc.RANDOM, 1] < 0
    assert pm.cell_of(*c["kps"][pc.RANDOM, KP["origin"]][["x", "y"]], c["bounds"][pc.RANDOM]) >= 0
    assert pm.cell_of(*c["kps"][pc.RANDOM, KP["origin"]][["x", "y"]], pc.BOUNDS[pc.PLANT]) != pm.cell_of(*c["kps"][pc.RANDOM, KP["origin"]][["x", "y"]], c["bounds"][pc.RANDOM])
    for b in (pc.I_RAND0, pc.I_RAND1):
        assert int(bound[b, P["origin", b]]) == KP["origin"]


def LIMITS_ARE(c):
    it = c["items"]
    return (it[pc.I_PLANT0]["max_dist"] == F(64.0) and it[pc.I_PLANT1]["max_dist"] == F(F(50) * F(1.5)) == F(75.0)
            and it[pc.I_RAND0]["max_dist"] == F(100.0) and it[pc.I_RAND3]["max_dist"] == F(50.0))


def test_the_planted_th_and_size_cases_are_what_they_claim(case):
    c = case
    P, KP = pc.PLANTED, pc.KP
    nm, match, bound, _ = c["want", True]
    sf = c["sf"]
    # (i) th 3, 5, 8 and 10 at level 6: the keypoint at x = th * sf exactly is no candidate, the float below it is; the product is rounded
    # to float32 for 3, 5 and 10 (8 * sf is exact)
    kinds = {}
    for th, b in pc.TH_ITEMS.items():
        it = c["items"][b]
        r = pm.radius_of(th, pc.TH_LEVEL, sf)
        assert it["th"] == F(th) and c["points"][b, P["th_at", th]]["u"] == 0 and c["points"][b, P["th_at", th]]["level"] == pc.TH_LEVEL
        assert c["kps"][pc.DENSE, KP["th_at", th]]["x"] == r and c["kps"][pc.DENSE, KP["th_inside", th]]["x"] == np.nextafter(r, F(0))
        assert (float(r) != float(F(th)) * float(sf[pc.TH_LEVEL])) == (th != 8.0), th
        assert int(bound[b, P["th_at", th]]) == -1 and int(bound[b, P["th_inside", th]]) == KP["th_inside", th] and nm[b] == 1, th
        kinds[th] = int(it["kind"])
    assert kinds == {3.0: pc.RELOC, 5.0: pc.SIM3, 8.0: pc.SIM3, 10.0: pc.RELOC}
    # (j) the dense site: lists longer than the small room's surplus, the item's lists more than the small room holds
    n = int(c["counts"][pc.DENSE, 0])
    cells = pm.assign_grid(c["kps"][pc.DENSE, :n], c["bounds"][pc.DENSE])
    for b, longest in ((pc.I_DENSE0, 144), (pc.I_DENSE1, 144)):
        lens = [len(pm.candidates(c["kps"][pc.DENSE, :n], c["desc"][pc.DENSE, :n], cells, c["bounds"][pc.DENSE], p, c["pdesc"], sf, c["items"][b]))
                for p in c["points"][b, :c["npts"][b]]]
        assert max(lens) == longest > pc.SMALL_ROOM and min(lens) > 64 and sum(lens) > 2 * (pc.SMALL_ROOM + pc.CAP), (b, lens)
        assert nm[b] >= 6
    assert not np.array_equal(match[pc.I_DENSE0], match[pc.I_DENSE1])
    # the sizes and the malformed kinds
    assert c["counts"][pc.EMPTY, 0] == 0 and c["npts"][pc.I_EMPTYFRAME] > 0 and nm[pc.I_EMPTYFRAME] == 0
    assert c["npts"][pc.I_NOPOINTS] == 0 and nm[pc.I_NOPOINTS] == 0
    assert c["npts"][pc.I_RAND1] % 64 and c["npts"][pc.I_RAND0] == pc.MCAP
    assert sorted(pc.MALFORMED.values()) == ["count", "frame", "kind", "level", "npts", "point", "th"]
    it = c["items"]
    assert it[21]["frame"] == pc.K and c["counts"][it[22]["frame"], 0] > pc.CAP and c["npts"][23] > pc.MCAP and it[24]["kind"] == 2
    assert not math.isfinite(it[25]["th"])
    assert (c["points"][26]["level"] == pc.NLEVELS).sum() == 1 and (c["points"][27]["point"] == len(c["pdesc"])).sum() == 1
    for ori in ORI:
        for b in pc.MALFORMED:
            assert c["want", ori][0][b] == -1 and (c["want", ori][1][b] == -1).all(), b
    # each malformed item is malformed by its one value alone: the row it copies is well-formed
    assert nm[pc.I_RAND0] > 0 and all(np.array_equal(c["kp_taken"][b], c["kp_taken"][pc.I_RAND0]) for b in pc.MALFORMED)


def test_the_planted_histogram_cases_are_what_they_claim(case):
    c = case
    P = pc.PLANTED
    nm, match, bound, bins = c["want", True]
    free = c["want", False]
    counts = lambda b: np.bincount(bins[b][bins[b] >= 0], minlength=30).tolist()   # noqa: E731
    # ties between bins: the first three in bin order stay
    h = counts(pc.I_TIES)
    assert [h[k] for k in (2, 5, 7, 9)] == [3, 3, 3, 3] and sum(h) == 12 and pm.three_maxima(h) == (2, 5, 7)
    assert nm[pc.I_TIES] == 9 and (match[pc.I_TIES] == -2).sum() == 3 and free[0][pc.I_TIES] == 12
    # max2 exactly at 0.1f * max1: kept
    h = counts(pc.I_TENTH)
    assert (h[4], h[1], h[8], h[11]) == (10, 1, 1, 1) and F(0.1) * F(10) == F(1.0) and pm.three_maxima(h) == (4, 1, 8)
    k = lambda b, name: int(bound[b, P[name]])   # noqa: E731
    assert match[pc.I_TENTH, k(pc.I_TENTH, ("tenth", 1))] >= 0 and match[pc.I_TENTH, k(pc.I_TENTH, ("tenth", 8))] >= 0
    assert match[pc.I_TENTH, k(pc.I_TENTH, ("tenth", 11))] == -2 and nm[pc.I_TENTH] == 12
    # max3 below 0.1f * max1: dropped; max2 above it: kept
    h = counts(pc.I_THIRD)
    assert (h[3], h[6], h[10]) == (20, 5, 1) and pm.three_maxima(h) == (3, 6, -1) and F(1) < F(0.1) * F(20) < F(5)
    assert match[pc.I_THIRD, k(pc.I_THIRD, ("third", 10))] == -2 and nm[pc.I_THIRD] == 25
    # rot exactly 0, the wrapped bin 30, a negative rot, no bin
    b = pc.I_ROT
    h = counts(b)
    assert (h[5], h[6], h[7], h[0], h[12]) == (8, 6, 5, 2, 1) and pm.three_maxima(h) == (5, 6, 7)
    pt = c["points"][b]
    assert bins[b, P["rot_zero"]] == 0 and pt[P["rot_zero"]]["angle"] == c["kps"][pc.HIST, k(b, "rot_zero")]["angle"]
    assert bins[b, P["rot_wrap"]] == 0 and round(float(F(F(900.0) * F(F(1.0) / F(30))))) == 30
    assert bins[b, P["rot_negative"]] == 12 and pt[P["rot_negative"]]["angle"] < c["kps"][pc.HIST, k(b, "rot_negative")]["angle"]
    assert bins[b, P["no_bin"]] == -1 and pm.rot_bin(2000.0, 0.0) == -1
    for name in ("rot_zero", "rot_wrap", "rot_negative"):
        assert match[b, k(b, name)] == -2, name
    assert match[b, k(b, "no_bin")] == P["no_bin"]                                            # never removed
    assert nm[b] == free[0][b] - 3 == (bound[b] >= 0).sum() - 3 and (match[b] == -2).sum() == 3
    # the same row under kind 1: no histogram, nothing removed, whatever check_orientation says
    s = pc.I_ROT_SIM3
    for key in ("u", "v", "angle", "level", "valid"):
        assert np.array_equal(c["points"][s][key], c["points"][b][key]), key
    assert np.array_equal(c["pdesc"][c["points"][s]["point"]], c["pdesc"][c["points"][b]["point"]])
    assert c["items"][s]["kind"] == pc.SIM3 and c["items"][s]["frame"] == c["items"][b]["frame"] and c["items"][s]["th"] == c["items"][b]["th"]
    assert nm[s] == free[0][s] == free[0][b] == 23 and np.array_equal(match[s], free[1][s]) and np.array_equal(match[s], free[1][b])
    assert (bins[s] == -1).all() and not (match[s] == -2).any()


def test_the_conditions_on_the_batch(case):
    """The batch's statistical floor, on the model: the GPU test cannot pass on an empty batch."""
    c = case
    good = good_items(c)
    on, off = c["want", True], c["want", False]
    kind = c["items"]["kind"]
    assert sum(int(on[0][b]) for b in good) >= 300 and sum(int(off[0][b]) for b in good) >= 300
    removed = {b: int((on[1][b] == -2).sum()) for b in good}
    assert sum(removed[b] for b in good if kind[b] == pc.RELOC) >= 1 and all(removed[b] == 0 for b in good if kind[b] == pc.SIM3)
    assert all(removed[b] > 0 for b in (pc.I_RAND0, pc.I_RAND2)) and not (off[1] == -2).any()
    assert all(on[0][b] == off[0][b] - removed[b] for b in good)
    for k in (pc.RELOC, pc.SIM3):
        assert sum(int(on[0][b]) for b in good if kind[b] == k) >= 100, k
    # the second copy of a doubled point falls to another keypoint or to none: the chain matters on the derived items
    nochain = 0
    for b in (pc.I_RAND0, pc.I_RAND1, pc.I_RAND2, pc.I_RAND3):
        bd = off[2][b][off[2][b] >= 0]
        assert len(np.unique(bd)) == len(bd)
        nochain += len(bd)
    assert nochain > 250
    assert len(good) == 21 and pc.B == 28
