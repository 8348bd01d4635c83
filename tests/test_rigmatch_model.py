"""tests/rigmatch_model.py and tests/rigmatch_cases.py held to their claims on the CPU: the constructed batch plants what it says it
plants, on the model's trace, and overflows the candidate room the GPU test's small-room path leaves."""
import numpy as np
import pytest

from tests import rigmatch_cases as rc
from tests import rigmatch_model as rm


@pytest.fixture(scope="module")
def case():
    c = rc.build()
    for th in rc.TH:
        c["local", th] = rm.search_local(c["side"], c["frames"], c["mp"], c["nmp"], c["pdesc"], c["sf"], th, rc.NN_RATIO, c["kp_obs"])
    for ori in (True, False):
        c["last", ori] = rm.search_last(c["side"], c["items"], c["pts"], c["nlast"], c["pdesc"], c["sf"], ori, c["kp_obs2"])
    return c


def test_the_planted_cases_are_what_they_claim(case):
    c = case
    L, P, P2, KL, KR = rc.CAP_L, rc.PLANTED, rc.PLANTED2, rc.KPL, rc.KPR
    n1, match1, obs1, trace1 = c["local", 1.0]
    n3, match3, _, trace3 = c["local", 3.0]
    t = trace1[rc.I_PLANT]
    # a left accept cross-binds through l2r onto a hidden right slot; the slot now holds the point and its obs
    assert c["kp_obs"][rc.I_PLANT, L + KR["cross"]] > 0
    assert t[P["cross_hidden"]]["left"] == ("accept", KL["cross"], L + KR["cross"], True) and t[P["cross_hidden"]]["right"] is None
    assert match1[rc.I_PLANT, L + KR["cross"]] == P["cross_hidden"] and obs1[rc.I_PLANT, L + KR["cross"]] == 2
    # the same with obs == 0 reopens the slot; a later point takes it, and binds r2l back onto the (open) left keypoint
    assert c["mp"][rc.I_PLANT, P["reopens"]]["obs"] == 0 and c["kp_obs"][rc.I_PLANT, L + KR["reopen"]] > 0
    assert t[P["reopens"]]["left"] == ("accept", KL["reopen"], L + KR["reopen"], True)
    assert P["takes_reopened"] > P["reopens"] and t[P["takes_reopened"]]["right"] == ("accept", L + KR["reopen"], KL["reopen"], False)
    assert match1[rc.I_PLANT, L + KR["reopen"]] == match1[rc.I_PLANT, KL["reopen"]] == P["takes_reopened"]
    # with a positive obs in its place the later point finds the slot hidden
    again = c["mp"].copy()
    again[rc.I_PLANT, P["reopens"]]["obs"] = 1
    t_again = rm.search_local(c["side"], c["frames"], again, c["nmp"], c["pdesc"], c["sf"], 1.0, rc.NN_RATIO, c["kp_obs"])[3][rc.I_PLANT]
    assert t_again[P["takes_reopened"]]["right"] == "none"
    # the :126 exit suppresses a right block that would have matched
    assert t[P["early_exit"]]["left"] == "ratio" and t[P["early_exit"]]["right"] is None
    again = c["mp"].copy()
    again[rc.I_PLANT, P["early_exit"]]["in_view"] = 0
    t_again = rm.search_local(c["side"], c["frames"], again, c["nmp"], c["pdesc"], c["sf"], 1.0, rc.NN_RATIO, c["kp_obs"])[3][rc.I_PLANT]
    assert t_again[P["early_exit"]]["right"] == ("accept", L + KR["early_exit"], None, False) and match1[rc.I_PLANT, L + KR["early_exit"]] == -1
    # a left empty list with a right match (entry 1); the same point shape ends at :1735 (entry 2)
    assert t[P["left_empty"]]["left"] == "empty" and t[P["left_empty"]]["right"] == ("accept", L + KR["left_empty"], None, False)
    n_l, match_l, obs_l, trace_l = c["last", True]
    t2 = trace_l[rc.J_NEITHER]["points"]
    assert t2[P2["left_empty"]] == dict(left="empty", right=None, lists=[0, 0]) and match_l[rc.J_NEITHER, L + KR["left_empty"]] == -1
    # level_r == -1
    assert t[P["level_r_none"]] == dict(left=None, right=None, lists=[0, 0]) and c["mp"][rc.I_PLANT, P["level_r_none"]]["in_view_r"] == 1
    # th != 1 leaves the right radius alone
    assert t[P["th"]]["left"] == "empty" and t[P["th"]]["right"] == "empty"
    assert trace3[rc.I_PLANT][P["th"]]["left"] == ("accept", KL["th"], None, False) and trace3[rc.I_PLANT][P["th"]]["right"] == "empty"
    # the float32(0.998) edge on view_cos_r
    assert t[P["cos_edge_r"]]["right"] == "empty" and t[P["cos_below_r"]]["right"] == ("accept", L + KR["cos_below_r"], None, False)
    # a right block hidden by its own point's left cross-binding
    own = t[P["own_cross_hides_right"]]
    assert own["left"] == ("accept", KL["own"], L + KR["own"], False) and own["right"] == "none" and own["right_hidden"] == [L + KR["own"]]
    assert c["kp_obs"][rc.I_PLANT, L + KR["own"]] == -1
    # r2l overwrites a pre-bound left slot
    assert c["kp_obs"][rc.I_PLANT, KL["r2l"]] > 0 and t[P["r2l_overwrites"]]["right"] == ("accept", L + KR["r2l"], KL["r2l"], True)
    assert match1[rc.I_PLANT, KL["r2l"]] == P["r2l_overwrites"] and obs1[rc.I_PLANT, KL["r2l"]] == 2
    # a keypoint outside the grid is no candidate, a non-finite projection has none, a point in neither view is not looked at
    assert t[P["outside"]]["left"] == "empty" and t[P["outside"]]["right"] == "empty" and t[P["nan_r"]]["right"] == "empty"
    assert P["neither"] not in t
    # one point leaves two histogram entries, in a kept and in a removed bin
    tr = trace_l[rc.J_NEITHER]
    two = [(slot, b) for q, slot, b in tr["entries"] if q == P2["two_entries"]]
    assert two == [(KL["two"], 0), (L + KR["two"], 3)] and tr["kept"] == (0, -1, -1)
    assert match_l[rc.J_NEITHER, KL["two"]] == P2["two_entries"] and match_l[rc.J_NEITHER, L + KR["two"]] == -2
    assert obs_l[rc.J_NEITHER, L + KR["two"]] == -1 and c["last", False][1][rc.J_NEITHER, L + KR["two"]] == P2["two_entries"]
    assert n_l[rc.J_NEITHER] == c["last", False][0][rc.J_NEITHER] - 1
    # directions 1 and 2 at octave 0
    assert c["pts"][rc.J_NEITHER, P2["direction"]]["octave"] == 0
    for j, name in ((rc.J_NEITHER, "dir_o0"), (rc.J_FORWARD, "dir_o3"), (rc.J_BACKWARD, "dir_o0")):
        tp = trace_l[j]["points"][P2["direction"]]
        assert tp["left"] == ("accept", KL[name]) and tp["right"] == ("accept", L + KR[name]), j
    assert trace_l[rc.J_NEITHER]["points"][P2["hidden"]]["left"] == ("accept", KL["runner_up2"]) and P2["invalid"] not in trace_l[rc.J_NEITHER]["points"]
    # an empty right frame
    assert c["side"]["counts_r"][rc.EMPTY_R, 0] == 0 and n1[rc.I_EMPTY_R] == 10 and n_l[rc.J_EMPTY_R] == 10
    assert (match1[rc.I_EMPTY_R, L:] == -1).all() and n1[rc.I_NOPOINTS] == 0
    # each malformed kind
    for b in rc.MALFORMED:
        assert n1[b] == n3[b] == -1 and (match1[b] == -1).all() and np.array_equal(obs1[b], c["kp_obs"][b]), b
    for b in rc.MALFORMED2:
        assert n_l[b] == -1 and (match_l[b] == -1).all() and np.array_equal(obs_l[b], c["kp_obs2"][b]), b
    assert (n1[:5] >= 0).all() and (n_l[:5] >= 0).all() and n1[rc.I_DENSE] > 20 and n_l[rc.J_DENSE] > 20
    kinds, frames, mp, nmp = rc.malformed_local(c)
    assert (rm.search_local(c["side"], frames, mp, nmp, c["pdesc"], c["sf"], 1.0, rc.NN_RATIO, np.zeros((len(kinds), rc.SLOTS), np.int32))[0] == -1).all()
    kinds, items, pts, nlast = rc.malformed_last(c)
    assert (rm.search_last(c["side"], items, pts, nlast, c["pdesc"], c["sf"], True, np.zeros((len(kinds), rc.SLOTS), np.int32))[0] == -1).all()
    # the dense items overflow the small room: several chunks; and one point's pair of lists always fits
    for trace, item in ((trace1[rc.I_DENSE], rc.I_DENSE), (trace_l[rc.J_DENSE]["points"], rc.J_DENSE)):
        lists = [sum(v["lists"]) for v in trace.values()]
        assert sum(lists) > 4 * rc.SMALL_ROOM and max(lists) <= rc.SLOTS <= rc.SMALL_ROOM, (item, sum(lists))
    assert len(c["frames"]) <= 8 and len(c["items"]) <= 8


# ---- the model held to the reference's recorded output (tests/golden/matcher_world_ref.txt.gz) on the dumped rig scenarios
def _model_on(rec):
    """{record name: (ret, ids)} of the model on a dump's three golden scenarios."""
    from tests import rigmatch_world as rw
    out = {}
    b = rw.local_batch(rec)
    n, match, _, _ = rm.search_local(b["side"], b["frames"], b["mp"], b["nmp"], b["pdesc"], b["sf"], b["th"], b["ratio"], b["kp_obs"])
    out["proj_mp_rig"] = (int(n[0]), rw.ids_line(b, match[0]))
    for name, wide in (("proj_last_rig", False), ("proj_last_rig_wide", True)):
        b = rw.last_batch(rec, "last.", wide)
        n, match, _, _ = rm.search_last(b["side"], b["items"], b["pts"], b["nlast"], b["pdesc"], b["sf"], True, b["kp_obs"])
        out[name] = (int(n[0]), rw.ids_line(b, match[0]))
    return out


def _same_records(got, want, names):
    for name in names:
        assert got[name][0] == want[name][0], (name, got[name][0], want[name][0])
        bad = np.nonzero(got[name][1] != want[name][1])[0]
        assert len(bad) == 0 and len(got[name][1]) == len(want[name][1]), (name, bad[:5].tolist())


RIG_RECORDS = ("proj_mp_rig", "proj_last_rig", "proj_last_rig_wide")


def test_the_model_equals_the_reference_on_the_recorded_rig_scenarios(tmp_path):
    import gzip
    import os
    from tests import rigmatch_world as rw
    from tests import world_util as wu
    gold = rw.golden_records(gzip.open(os.path.join(wu.ROOT, "tests", "golden", "matcher_world_ref.txt.gz")).read().decode())
    assert [gold[n][0] for n in RIG_RECORDS] == [rw.LOCAL_RET, 1189, 1500] and all(len(gold[n][1]) == 2015 for n in RIG_RECORDS)
    rec = rw.dump(rw.golden_world(tmp_path), tmp_path)
    assert int(rec["last.direction"][0]) == 0
    _same_records(_model_on(rec), gold, RIG_RECORDS)
    # the dump's frames are the scenarios': the drop-in adapter on them prints the same lines
    for name, b in (("proj_mp_rig", rw.local_batch(rec)), ("proj_last_rig", rw.last_batch(rec, "last."))):
        assert b["adapter"][0] == gold[name][0] and np.array_equal(b["adapter"][1], gold[name][1]), name


def test_the_model_equals_the_reference_on_another_world(tmp_path):
    import os
    from tests import rigmatch_world as rw
    from tests import world_util as wu
    from tests.test_matcher_world import OTHER_WORLDS
    if not os.path.exists(wu.REF_EXE):
        pytest.skip("oracle/_ref/ref_matcher_world not built (needs the reference)")
    kw = dict(OTHER_WORLDS[0], rows=512, cols=512, nfeatures=400)
    world = str(tmp_path / "world.bin")
    wu.write_world(world, **kw)
    ref = rw.golden_records(wu.run_world(wu.REF_EXE, world, str(tmp_path / "ref.txt"), only="proj_"))
    assert ref["proj_mp_rig"][0] > 50 and ref["proj_last_rig"][0] > 100
    _same_records(_model_on(rw.dump(world, tmp_path)), ref, RIG_RECORDS)


@pytest.mark.parametrize("tag,direction", (("forward.", 1), ("backward.", 2)))
def test_directions_1_and_2_equal_the_adapter(tmp_path, tag, direction):
    """The golden covers only the "neither" direction on a rig.  This leg rests on the drop-in adapter (oracle backend), whose direction
    switch the reference holds on stereo frames (proj_last_stereo_forward / _backward of the same golden), run on the proj_last_rig frames
    with a forward (tz = -0.3f) and a backward (tz = 0.3f) pose."""
    from tests import rigmatch_world as rw
    rec = rw.dump(rw.golden_world(tmp_path), tmp_path)
    assert int(rec[tag + "direction"][0]) == direction
    b = rw.last_batch(rec, tag)
    n, match, _, _ = rm.search_last(b["side"], b["items"], b["pts"], b["nlast"], b["pdesc"], b["sf"], True, b["kp_obs"])
    assert b["adapter"][0] > 100 and int(n[0]) == b["adapter"][0]
    assert np.array_equal(rw.ids_line(b, match[0]), b["adapter"][1])
