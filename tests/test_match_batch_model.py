"""tests/match_batch_model.py, the plain statement of the batched SearchByBoW: in frame mode it is held to the oracle's SearchByBoW on
oracle-extracted frames; the keyframe mode, which the oracle has no array-level routine for, to hand cases (CPU only)."""
import numpy as np
import pytest

from oracle import pyoracle as po
from orb_slam3_modified_amd import synth
from tests import match_batch_model as mm
from tests.vocab_util import make_vocabulary


@pytest.fixture(scope="module")
def frames(tmp_path_factory):
    ex = po.OracleExtractor(1000, 1.2, 8, 20, 7)
    imgs = synth.make_stream(6, 480, 640, 4242)
    out = []
    for f in (0, 1, 5):
        kps, desc, _ = ex.extract(imgs[f], (0, 1000))
        out.append((kps, desc))
    p = str(tmp_path_factory.mktemp("voc") / "voc.txt")
    make_vocabulary(p, np.concatenate([d for _, d in out]), 10, 4, seed=5)
    return out, po.OracleVocabulary(p)


@pytest.mark.parametrize("levelsup", [0, 2, 4])
@pytest.mark.parametrize("ratio,ori", [(0.6, True), (0.7, False), (0.9, True)])
def test_frame_mode_equals_the_oracle(frames, levelsup, ratio, ori):
    fr, ov = frames
    rng = np.random.default_rng(levelsup * 10 + int(ratio * 10))
    fvs = [ov.transform(d, levelsup)[1] for _, d in fr]
    total = removed = contended = 0
    for ia, ib in ((0, 1), (0, 2), (1, 1), (2, 0)):
        (ka, da), (kb, db) = fr[ia], fr[ib]
        for valid in (np.ones(len(da), np.uint8), (rng.random(len(da)) < 0.7).astype(np.uint8)):
            on, ob2a = po.search_by_bow(da, ka["angle"], valid, fvs[ia], db, kb["angle"], fvs[ib], ratio, ori)
            st = {}
            n, b2a = mm.search_by_bow(da, ka["angle"], valid, fvs[ia], db, kb["angle"], None, fvs[ib], mm.FRAME, ratio, ori, stats=st)
            assert n == on and np.array_equal(b2a, ob2a), (ia, ib, levelsup, ratio, ori)
            a2b = mm.invert(b2a, len(da))
            assert (a2b >= 0).sum() == n and all(b2a[a2b[i]] == i for i in np.nonzero(a2b >= 0)[0])
            total += on
            removed += st["removed"]
            contended += st["contended"]
    assert total > 100 and contended > 0
    if ori:
        assert removed > 0


def _desc(bits):
    """A descriptor with the first `bits` bits set."""
    d = np.zeros(32, np.uint8)
    d[:bits // 8] = 0xFF
    if bits % 8:
        d[bits // 8] = (1 << (bits % 8)) - 1
    return d


def test_a_best_distance_of_exactly_fifty():
    """<= 50 towards a frame, < 50 between keyframes."""
    da, db = np.stack([_desc(0)]), np.stack([_desc(50), _desc(200)])
    ang = np.zeros(2, np.float32)
    fv = {3: [0]}, {3: [0, 1]}
    n, b2a = mm.search_by_bow(da, ang[:1], None, fv[0], db, ang, None, fv[1], mm.FRAME, 0.7, False)
    assert n == 1 and b2a.tolist() == [0, -1]
    on, ob2a = po.search_by_bow(da, ang[:1], np.ones(1, np.uint8), fv[0], db, ang, fv[1], 0.7, False)
    assert on == 1 and ob2a.tolist() == [0, -1]
    n, b2a = mm.search_by_bow(da, ang[:1], None, fv[0], db, ang, None, fv[1], mm.KEYFRAMES, 0.7, False)
    assert n == 0 and b2a.tolist() == [-1, -1]
    db[0] = _desc(49)
    n, b2a = mm.search_by_bow(da, ang[:1], None, fv[0], db, ang, None, fv[1], mm.KEYFRAMES, 0.7, False)
    assert n == 1 and b2a.tolist() == [0, -1]


def test_an_invalid_b_feature_that_would_have_been_the_best():
    da = np.stack([_desc(0)])
    db = np.stack([_desc(5), _desc(30), _desc(120)])
    ang = np.zeros(3, np.float32)
    fa, fb = {9: [0]}, {9: [0, 1, 2]}
    valid_b = np.array([0, 1, 1], np.uint8)
    n, b2a = mm.search_by_bow(da, ang[:1], None, fa, db, ang, valid_b, fb, mm.KEYFRAMES, 0.7, False)
    assert n == 1 and b2a.tolist() == [-1, 0, -1]           # 30 < 0.7 * 120
    n, b2a = mm.search_by_bow(da, ang[:1], None, fa, db, ang, valid_b, fb, mm.FRAME, 0.7, False)
    assert n == 1 and b2a.tolist() == [0, -1, -1]           # a frame's features are all candidates
    n, b2a = mm.search_by_bow(da, ang[:1], None, fa, db, ang, None, fb, mm.KEYFRAMES, 0.7, False)
    assert n == 1 and b2a.tolist() == [0, -1, -1]
    # the invalid feature does not serve as second best either: 30 against 40 fails the ratio, against nothing else it would pass
    db[2] = _desc(40)
    n, _ = mm.search_by_bow(da, ang[:1], None, fa, db, ang, valid_b, fb, mm.KEYFRAMES, 0.7, False)
    assert n == 0


def test_taken_features_ties_and_the_rotation_filter():
    # two A features want B feature 0; the first takes it, the second falls back on B feature 1 (second best 256: nothing else is left)
    da = np.stack([_desc(0), _desc(1)])
    db = np.stack([_desc(0), _desc(8)])
    ang0 = np.zeros(2, np.float32)
    fa, fb = {1: [0, 1]}, {1: [0, 1]}
    n, b2a = mm.search_by_bow(da, ang0, None, fa, db, ang0, None, fb, mm.FRAME, 0.7, False)
    assert n == 2 and b2a.tolist() == [0, 1]
    on, ob2a = po.search_by_bow(da, ang0, np.ones(2, np.uint8), fa, db, ang0, fb, 0.7, False)
    assert (on, ob2a.tolist()) == (n, b2a.tolist())
    # a tie of the two smallest distances: second best = best, the ratio test fails
    db2 = np.stack([_desc(8), _desc(8)])
    n, _ = mm.search_by_bow(da[:1], ang0[:1], None, {1: [0]}, db2, ang0, None, fb, mm.FRAME, 0.9, False)
    assert n == 0
    # twelve matches rotate by about 0 degrees, one by 90: the lone bin holds less than a tenth of the first and is removed
    k = 13
    da = np.stack([np.full(32, i, np.uint8) for i in range(k)])
    fa = {i: [i] for i in range(k)}
    aa, ab = np.full(k, 100.0, np.float32), np.full(k, 100.0, np.float32)
    ab[5] = 10.0
    st = {}
    n, b2a = mm.search_by_bow(da, aa, None, fa, da, ab, None, fa, mm.KEYFRAMES, 0.7, True, stats=st)
    assert n == k - 1 and b2a[5] == -1 and st["removed"] == 1
    on, ob2a = po.search_by_bow(da, aa, np.ones(k, np.uint8), fa, da, ab, fa, 0.7, True)
    assert on == n and np.array_equal(ob2a, b2a)
    assert mm.rotation_bin(10.0, 25.0) == 12 and mm.rotation_bin(359.0, 0.0) == 12 and mm.rotation_bin(0.0, 1.0) == 12
    assert mm.rotation_bin(15.0, 0.0) == 1 and mm.rotation_bin(14.9, 0.0) == 0 and mm.rotation_bin(0.0, 346.0) == 0


# ---- the constructed batch of tests/match_batch_cases.py, held to the oracle (frame mode) and to its own claims
from tests import match_batch_cases as mc  # noqa: E402

F32 = np.float32
COMBOS = [(mode, valid, ori) for mode in (mm.FRAME, mm.KEYFRAMES) for valid in (True, False) for ori in (True, False)]


@pytest.fixture(scope="module")
def case():
    """The batch and -- computed once -- the model's (nmatches, b2a) of every well-formed pair under every run, mode, valid form and
    check_orientation."""
    c = mc.build()
    for run, ratio in mc.RUNS.items():
        for mode, valid, ori in COMBOS:
            for p, (ia, ib) in enumerate(mc.PAIRS.tolist()):
                if p not in mc.MALFORMED:
                    (da, aa, va, fa), (db, ab, vb, fb) = mc.frame(c, ia), mc.frame(c, ib)
                    c["want", run, mode, valid, ori, p] = mm.search_by_bow(da, aa, va if valid else None, fa, db, ab, vb if valid else None, fb, mode, ratio, ori)
    return c


@pytest.mark.parametrize("run", list(mc.RUNS))
def test_the_model_is_the_oracle_on_the_constructed_batch(case, run):
    """Frame mode only: the oracle's SearchByBoW(KeyFrame, Frame) takes hand-built FeatureVectors, a keyframe-mode routine it has not."""
    c = case
    for p, (ia, ib) in enumerate(mc.PAIRS.tolist()):
        if p in mc.MALFORMED:
            continue
        (da, aa, va, fa), (db, ab, _, fb) = mc.frame(c, ia), mc.frame(c, ib)
        for valid in (True, False):
            for ori in (True, False):
                on, ob2a = po.search_by_bow(da, aa, va if valid else np.ones(len(da), np.uint8), fa, db, ab, fb, mc.RUNS[run], ori)
                n, b2a = c["want", run, mm.FRAME, valid, ori, p]
                assert n == on and np.array_equal(b2a, ob2a), (run, p, valid, ori)


def test_the_planted_nodes_are_what_they_claim(case):
    c = case
    for name, (p, run, want) in mc.CLAIMS.items():
        na = int(c["counts"][mc.PAIRS[p, 0], 0])
        for mode, valid, ori in COMBOS:
            if p in (mc.P_ROT1, mc.P_ROT2) and not ori:
                expect = mc.KP[name]                              # without the filter every rotation site keeps its match
            else:
                w = want(mode, valid)
                expect = -1 if w is None else mc.KP[w]
            held = int(mm.invert(c["want", run, mode, valid, ori, p][1], na)[mc.PLANTED[name]])
            assert held == expect, (name, mode, valid, ori, held, expect)
    assert mc.KP["tie"] > mc.KP["tie:lower_index"]               # fv_feat order, not index order
    fa = c["fv"][mc.MA]
    assert any(l != sorted(l) for l in fa.values()) and any(l != sorted(l) for l in c["fv"][mc.MB].values())
    assert mc.PLANTED["first_takes"] > mc.PLANTED["runner_up"]
    assert c["valid"][mc.MA, mc.PLANTED["invalid_a"]] == 0 and c["valid"][mc.MB, mc.KP["invalid_b_best"]] == 0
    # the node lists
    nodes = lambda f: set(c["fv"][f])   # noqa: E731
    assert not nodes(mc.E1) & nodes(mc.E2) and nodes(mc.E1) & nodes(mc.E3) == {min(nodes(mc.E1))} and nodes(mc.E1) & nodes(mc.E5) == {max(nodes(mc.E1))}
    assert c["fv_n"][mc.NOFV] == 0 and nodes(mc.WA) - nodes(mc.WB1) and nodes(mc.MA) - nodes(mc.MB) and nodes(mc.MB) - nodes(mc.MA)
    one_sided = min(nodes(mc.MA) - nodes(mc.MB))
    assert min(nodes(mc.MA) & nodes(mc.MB)) < one_sided < max(nodes(mc.MA) & nodes(mc.MB))
    # the malformed pairs, exactly as the header lists them
    assert sorted(mc.MALFORMED.values()) == ["frame", "fv_feat entry at its frame's count", "negative count", "negative fv_n"]
    assert c["counts"][mc.NEGCOUNT, 0] < 0 and c["fv_n"][mc.NEGFV] < 0 and not 0 <= mc.PAIRS[mc.P_BADFRAME, 1] < mc.K
    f = mc.BADFEAT
    assert (c["fv_feat"][f, :c["fv_ptr"][f, c["fv_n"][f]]] >= c["counts"][f, 0]).sum() == 1
    # the arrays say what the dicts say
    for f in range(mc.K):
        k = max(int(c["fv_n"][f]), 0) if f != mc.NEGFV else len(c["fv"][f])
        got = {int(c["fv_node"][f, j]): c["fv_feat"][f, c["fv_ptr"][f, j]:c["fv_ptr"][f, j + 1]].tolist() for j in range(k)}
        if f != mc.BADFEAT:
            assert got == c["fv"][f] and list(got) == sorted(got), f


def test_the_float32_facts_the_nodes_rest_on():
    best, second, ratio = mc.BEST, mc.SECOND, mc.RATIO
    assert F32(ratio) * F32(second) == F32(best) and not F32(best) < F32(ratio) * F32(second) and best < 50
    assert float(best) < float(F32(ratio)) * second and F32(best - 1) < F32(ratio) * F32(second)
    assert F32(25) < F32(0.1) * F32(256) and not F32(26) < F32(0.1) * F32(256)          # 256, not INT_MAX, is a lone candidate's second
    assert not F32(256) < F32(1.5) * F32(256) or 256 > 50
    assert F32(0.1) * F32(30) == F32(3.0) and float(F32(0.1)) * 30 > 3.0
    assert mm.three_maxima([30, 3, 2] + [0] * 27) == [0, 1, -1] and mm.three_maxima([2, 0, 0, 2, 0, 0, 2, 0, 0, 2] + [0] * 20) == [0, 3, 6]
    e11, e12 = mc.bin_edge(11)
    assert np.nextafter(e11, F32(400)) == e12 and (mm.rotation_bin(e11, 0.0), mm.rotation_bin(e12, 0.0)) == (11, 12)
    assert mm.rotation_bin(900.0, 0.0) == 0 and mm.rotation_bin(0.0, 5.0) == 12 and mm.rotation_bin(10.0, 20.0) == 12


def test_the_trips_of_the_batch(case):
    """The list lengths and positions the wave-node sites rest on: 63 and 64 candidates stay in registers, 65 and 129 take two and three
    trips; the twice-standing minimum's later position sits on the lower lane of a later trip."""
    c = case
    sizes = {name: len(c["fv"][f][n]) for name, f, n in (("nb_1", mc.WB1, 100), ("nb_63", mc.WB1, 163), ("nb_64", mc.WB1, 164), ("nb_65", mc.WB1, 165),
                                                           ("nb_129", mc.WB2, 229), ("lane_pair", mc.WB2, 172), ("lane_pair_twin", mc.WB3, 173))}
    assert sizes == mc.N_WAVE
    for name, f, n in (("nb_63", mc.WB1, 163), ("nb_64", mc.WB1, 164), ("nb_65", mc.WB1, 165), ("nb_129", mc.WB2, 229)):
        lst, (lo, hi) = c["fv"][f][n], mc.KP[name + ":positions"]
        dist = [int(np.unpackbits(c["desc"][f, i]).sum()) for i in lst]           # the query is desc(0)
        assert [j for j, d in enumerate(dist) if d == min(dist)] == [lo, hi] and lst[lo] == mc.KP[name] and lst[hi] == mc.KP[name + ":later"]
        assert lst == sorted(lst, reverse=True)                   # positions run against the indices
        if len(lst) > 64:
            assert lo // 64 != hi // 64 and hi % 64 < lo % 64
    for f, n, second in ((mc.WB2, 172, 22), (mc.WB3, 173, 100)):
        dist = [int(np.unpackbits(c["desc"][f, i]).sum()) for i in c["fv"][f][n]]
        assert dist[7] == 20 == min(dist) and dist[71] == second == sorted(dist)[1] and 7 % 64 == 71 % 64
        assert (F32(20) < F32(mc.RATIO) * F32(second)) == (second == 100) and F32(20) < F32(mc.RATIO) * F32(sorted(dist)[2])
    # the long chain: 70 A features over 4 candidates, four matches, and 66 A features find every candidate taken
    assert len(c["fv"][mc.WA][300]) == 70 and len(c["fv"][mc.WB3][300]) == 4
    n, b2a = c["want", "main", mm.FRAME, False, False, mc.P_W3]
    assert sorted(b2a[c["fv"][mc.WB3][300]].tolist()) == sorted(c["fv"][mc.WA][300][:4]) and n == 5
