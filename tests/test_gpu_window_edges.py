"""The chain core's size edges (csrc/side/orbx_window_device.h, orbx_window_host.h) on the GPU: the batches of tests/window_edge_cases.py
through the host forms of the four libraries on it (one batch through the device forms of the first two), on the paths each batch names.
liborbx_lastmatch.so and liborbx_localmatch.so: for every item (nmatches, kp_match, kp_obs) equals the compiled oracle's, called per item
on the item's frame.  liborbx_projmatch.so and liborbx_rigmatch.so (both entries): the rows of tests/projmatch_model.py and
tests/rigmatch_model.py, at the reduced sizes.  Whole rows, the tail beyond n included; a malformed item gives -1, a row of -1 and kp_obs
as it was.  tests/test_window_edge_cases.py holds the batches to the sizes and claims that make them edges."""
import numpy as np
import pytest

from orb_slam3_modified_amd.lastmatch import LastMatchBatch, LastMatchSide
from orb_slam3_modified_amd.localmatch import LocalMatchBatch, LocalMatchSide
from orb_slam3_modified_amd._window import LDS_MAX
from tests import window_edge_cases as wc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MATCHERS = ("last", "local")
ENV = {"last": "ORBX_LASTMATCH_LDS", "local": "ORBX_LOCALMATCH_LDS"}
VARIANTS = {"last": (True, False), "local": (None,)}             # the rotation check on and off; the local matcher has none
PATHS = pytest.mark.parametrize("lds", (None, 0), ids=("lds", "global"))


def _check(got, want, where):
    """Whole rows: nmatches [B], kp_match and kp_obs [B, cap]."""
    for g, w, name in zip(got, want, ("nmatches", "kp_match", "kp_obs")):
        g = np.asarray(g)
        assert g.shape == w.shape, (where, name, g.shape, w.shape)
        bad = np.nonzero(np.asarray(g != w).reshape(len(w), -1).any(1))[0]
        assert len(bad) == 0, (where, name, bad[:5].tolist())


def _handle(matcher, monkeypatch, lds):
    """A handle created under the LDS limit `lds` (None: the default)."""
    if lds is not None:
        monkeypatch.setenv(ENV[matcher], str(lds))
    h = LastMatchBatch(0) if matcher == "last" else LocalMatchBatch(0)
    monkeypatch.delenv(ENV[matcher], raising=False)
    return h


def _want(matcher, s, ori):
    return wc.want_last(s, ori) if matcher == "last" else wc.want_local(s)


def _search(h, matcher, s, ori):
    """The scene through the host form."""
    Side = LastMatchSide if matcher == "last" else LocalMatchSide
    side = Side(s["kps"], s["desc"], s["counts"], s["bounds"], s["K"], s["cap"], s["uright"])
    if matcher == "last":
        a = wc.as_last(s)
        r = h.search(side, a["items"], a["points"], a["nlast"], s["pdesc"], s["sf"], s["kp_obs"], ori)
    else:
        a = wc.as_local(s)
        r = h.search(side, a["frames"], a["mp"], a["nmp"], s["pdesc"], s["sf"], s["kp_obs"], a["th"], wc.NN_RATIO)
    return r.nmatches, r.kp_match, r.kp_obs


def _hold(h, matcher, s, where, want=None):
    """Every item of the scene against the reference, for each of the matcher's variants."""
    kept = s["kp_obs"].copy()
    for ori in VARIANTS[matcher]:
        w = want[ori] if want is not None else _want(matcher, s, ori)
        got = _search(h, matcher, s, ori)
        _check(got, w, (where, ori))
        for b in s["bad"]:                                        # -1, a row of -1, kp_obs as it was
            assert got[0][b] == -1 and (got[1][b] == -1).all() and np.array_equal(got[2][b], kept[b]), (where, b)
    assert np.array_equal(s["kp_obs"], kept)


# ---- batch 1: a workgroup walks several items
@pytest.fixture(scope="module")
def many():
    """The tiled batch and the reference's rows: computed once per pool entry and tiled (the items are independent)."""
    pool = wc.many_items_pool()
    idx = np.arange(wc.MANY) % wc.P
    want = {m: {ori: tuple(np.ascontiguousarray(r[idx]) for r in _want(m, pool, ori)) for ori in VARIANTS[m]} for m in MATCHERS}
    return wc.tile(pool, wc.MANY), want


@pytest.mark.parametrize("matcher", MATCHERS)
@PATHS
def test_many_items_through_the_host_form(many, monkeypatch, matcher, lds):
    s, want = many
    assert len(s["frame"]) == wc.MANY > 2 * wc.MAX_BLOCKS >= 8 * wc.GLOBAL_BLOCKS    # up to 3 items a workgroup on LDS, 8 to 9 on the global path
    h = _handle(matcher, monkeypatch, lds)
    _hold(h, matcher, s, ("many", lds), want[matcher])
    h.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@pytest.mark.parametrize("matcher", MATCHERS)
def test_many_items_through_the_device_form(many, matcher):
    s, want = many
    K, cap, B = s["K"], s["cap"], wc.MANY
    Side = LastMatchSide if matcher == "last" else LocalMatchSide
    side = Side(_dev(s["kps"].view(np.uint8).reshape(K, cap, -1)), _dev(s["desc"]), _dev(s["counts"]), _dev(s["bounds"]), K, cap, _dev(s["uright"]))
    pdesc = _dev(s["pdesc"])
    h = LastMatchBatch(0) if matcher == "last" else LocalMatchBatch(0)
    for ori in VARIANTS[matcher]:
        t_obs = _dev(s["kp_obs"])
        if matcher == "last":
            a = wc.as_last(s)
            out = h.search_device(side, _dev(a["items"].view(np.uint8).reshape(B, 16)), _dev(a["points"].view(np.uint8).reshape(B, -1, 32)),
                                  _dev(a["nlast"]), pdesc, s["sf"], t_obs, ori)
        else:
            a = wc.as_local(s)
            out = h.search_device(side, _dev(a["frames"]), _dev(a["mp"].view(np.uint8).reshape(B, -1, 32)), _dev(a["nmp"]), pdesc, s["sf"], t_obs,
                                  a["th"], wc.NN_RATIO)
        torch.cuda.synchronize()
        assert out.kp_obs is t_obs
        _check((out.nmatches.cpu().numpy(), out.kp_match.cpu().numpy(), t_obs.cpu().numpy()), want[matcher][ori], ("many, device form", ori))
    h.close()


# ---- batch 2: the sort's sizes
@pytest.mark.parametrize("matcher", MATCHERS)
@PATHS
def test_sort_sizes(monkeypatch, matcher, lds):
    h = _handle(matcher, monkeypatch, lds)
    _hold(h, matcher, wc.sort_sizes(), ("sort", lds))
    _hold(h, matcher, wc.sort_full(), ("sort, cap == n == p2", lds))
    h.close()


# ---- batch 3: the points' counts
@pytest.mark.parametrize("matcher", MATCHERS)
@PATHS
def test_point_counts(monkeypatch, matcher, lds):
    h = _handle(matcher, monkeypatch, lds)
    _hold(h, matcher, wc.point_counts(), ("points", lds))
    h.close()


# ---- batch 4 and 5 (a): list lengths and lanes; the chunk cut with room == cap, and the same batch on the global path 16 bytes below
LANES_LIMIT = wc.room_limit(wc.LANES_CAP, wc.LANES_MCAP, wc.LANES_CAP)


@pytest.mark.parametrize("matcher", MATCHERS)
@pytest.mark.parametrize("lds", (None, LANES_LIMIT, LANES_LIMIT - 16), ids=("lds", "room-is-cap", "global-below"))
def test_list_lanes_and_the_chunk_cut(monkeypatch, matcher, lds):
    assert wc.plan_room(LANES_LIMIT, wc.LANES_CAP, wc.LANES_MCAP) == wc.LANES_CAP and wc.plan_room(LANES_LIMIT - 16, wc.LANES_CAP, wc.LANES_MCAP) is None
    h = _handle(matcher, monkeypatch, lds)
    _hold(h, matcher, wc.list_lanes(), ("lanes", lds))
    h.close()


# ---- batch 5 (b): the global path's cut at kGlobalRoom
@pytest.mark.parametrize("matcher", MATCHERS)
def test_global_cut(monkeypatch, matcher):
    h = _handle(matcher, monkeypatch, 0)
    _hold(h, matcher, wc.global_cut(), "global cut")
    h.close()


# ---- batch 6: the default limit's switch
@pytest.mark.parametrize("matcher", MATCHERS)
def test_default_limit_switch(monkeypatch, matcher):
    c = wc.largest_lds_capacity()
    assert wc.plan_room(LDS_MAX, c, wc.SWITCH_MCAP) is not None and wc.plan_room(LDS_MAX, c + 1, wc.SWITCH_MCAP) is None
    h = _handle(matcher, monkeypatch, None)
    _hold(h, matcher, wc.limit_switch(c), ("switch", c))          # the full dynamic LDS block
    _hold(h, matcher, wc.limit_switch(c + 1), ("switch", c + 1))  # the global path
    h.close()


# ---- batch 7: capacity 32768
@pytest.mark.parametrize("matcher", MATCHERS)
def test_capacity_max(monkeypatch, matcher):
    s = wc.capacity_max()
    h = _handle(matcher, monkeypatch, None)
    _hold(h, matcher, s, "capacity 32768")
    got = _search(h, matcher, s, False)
    assert got[1][1, wc.MAX_CAP - 1] == 2 and got[1][0, wc.MAX_CAP - 1] == -1 and got[2][0, wc.MAX_CAP - 1] == 3
    h.close()


# ---- the model-checked matchers, ProjMatchBatch and RigMatchBatch (both entries), at the reduced sizes: whole rows against
# tests/projmatch_model.py and tests/rigmatch_model.py
from orb_slam3_modified_amd.projmatch import ProjMatchBatch, ProjMatchSide  # noqa: E402
from orb_slam3_modified_amd.rigmatch import RigMatchBatch, RigSide  # noqa: E402

ORI = (True, False)
RIG_RUNS = (("local", None), ("last", True), ("last", False))


def _proj_handle(monkeypatch, lds):
    if lds is not None:
        monkeypatch.setenv("ORBX_PROJMATCH_LDS", str(lds))
    h = ProjMatchBatch(0)
    monkeypatch.delenv("ORBX_PROJMATCH_LDS", raising=False)
    return h


def _rig_handle(monkeypatch, lds):
    if lds is not None:
        monkeypatch.setenv("ORBX_RIGMATCH_LDS", str(lds))
    h = RigMatchBatch(0)
    monkeypatch.delenv("ORBX_RIGMATCH_LDS", raising=False)
    return h


def _hold_proj(h, s, where, want=None):
    a = wc.as_proj(s)
    side = ProjMatchSide(s["kps"], s["desc"], s["counts"], s["bounds"], s["K"], s["cap"])
    for ori in ORI:
        w = want[ori] if want is not None else wc.model_proj(s, ori)[:2]
        r = h.search(side, a["items"], a["points"], a["npts"], s["pdesc"], s["sf"], a["kp_taken"], ori)
        _check((r.nmatches, r.kp_match), w, (where, ori))
        for b in s["bad"]:
            assert r.nmatches[b] == -1 and (r.kp_match[b] == -1).all(), (where, b)


def _hold_rig(h, r, where, want=None):
    side = RigSide(r["kps"], r["desc"], r["counts"], r["kps_r"], r["desc_r"], r["counts_r"], r["l2r"], r["r2l"], r["bounds"], r["K"], r["cap_l"], r["cap_r"])
    kept = r["kp_obs"].copy()
    for entry, ori in RIG_RUNS:
        w = want[entry, ori] if want is not None else wc.model_rig(r, entry, ori)[:3]
        if entry == "local":
            a = wc.as_rig_local(r)
            g = h.search_local_points(side, a["frames"], a["mp"], a["nmp"], r["pdesc"], r["sf"], r["kp_obs"], a["th"], wc.NN_RATIO)
        else:
            a = wc.as_rig_last(r)
            g = h.search_last_frame(side, a["items"], a["points"], a["nlast"], r["pdesc"], r["sf"], r["kp_obs"], ori)
        _check((g.nmatches, g.kp_match, g.kp_obs), w, (where, entry, ori))
        for b in r["bad"]:
            assert g.nmatches[b] == -1 and (g.kp_match[b] == -1).all() and np.array_equal(g.kp_obs[b], kept[b]), (where, b)
    assert np.array_equal(r["kp_obs"], kept)


@pytest.fixture(scope="module")
def many_models():
    """Batch 1 for the two model-checked matchers: the models' rows once per pool entry, tiled."""
    pool = wc.many_items_pool()
    rig = wc.rig_of(pool, cap_r=60)
    idx = np.arange(wc.MANY) % wc.P
    tiled = lambda rows: tuple(np.ascontiguousarray(x[idx]) for x in rows)   # noqa: E731
    return (wc.tile(pool, wc.MANY), {ori: tiled(wc.model_proj(pool, ori)[:2]) for ori in ORI},
            wc.tile(rig, wc.MANY), {(e, ori): tiled(wc.model_rig(rig, e, ori)[:3]) for e, ori in RIG_RUNS})


@PATHS
def test_proj_many_items(many_models, monkeypatch, lds):
    s, want, _, _ = many_models
    h = _proj_handle(monkeypatch, lds)
    _hold_proj(h, s, ("proj many", lds), want)
    h.close()


@PATHS
def test_rig_many_items(many_models, monkeypatch, lds):
    _, _, r, want = many_models
    h = _rig_handle(monkeypatch, lds)
    _hold_rig(h, r, ("rig many", lds), want)
    h.close()


@PATHS
def test_proj_sort_sizes_point_counts_and_lists(monkeypatch, lds):
    h = _proj_handle(monkeypatch, lds)
    _hold_proj(h, wc.sort_sizes(wc.PROJ_SORT_N0), ("proj sort", lds))
    _hold_proj(h, wc.point_counts(wc.PROJ_NLAST), ("proj points", lds))
    _hold_proj(h, wc.lanes_plain(), ("proj lists", lds))
    h.close()


@PATHS
def test_rig_sort_sizes_point_counts_and_lists(monkeypatch, lds):
    h = _rig_handle(monkeypatch, lds)
    _hold_rig(h, wc.rig_of(wc.sort_sizes(wc.PROJ_SORT_N0)), ("rig sort", lds))           # other in-grid counts on the second camera
    _hold_rig(h, wc.rig_of(wc.point_counts(wc.PROJ_NLAST)), ("rig points", lds))
    _hold_rig(h, wc.rig_of(wc.lanes_plain(), drop=lambda n: 0), ("rig lists", lds))
    h.close()


def test_rig_default_limit_switch(monkeypatch):
    from orb_slam3_modified_amd._window import rig_lds_bytes
    c, q = wc.largest_rig_lds_capacity(wc.RIG_SWITCH_MCAP), wc.RIG_SWITCH_MCAP
    assert rig_lds_bytes(c, c, q) + 8 * c <= LDS_MAX < rig_lds_bytes(c + 1, c + 1, q) + 8 * (c + 1)
    h = _rig_handle(monkeypatch, None)
    for cap in (c, c + 1):                                        # the full dynamic LDS block, then the global path
        _hold_rig(h, wc.rig_of(wc.limit_switch(cap, wc.RIG_SWITCH_POINTS, q), drop=lambda n: 0), ("rig switch", cap))
    h.close()


def test_rig_capacity_max(monkeypatch):
    r = wc.rig_capacity_max()
    assert r["cap_l"] + r["cap_r"] == wc.MAX_CAP
    h = _rig_handle(monkeypatch, None)
    _hold_rig(h, r, "rig 16384 + 16384")
    h.close()
