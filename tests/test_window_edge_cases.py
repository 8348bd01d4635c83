"""tests/window_edge_cases.py held to its claims, without a GPU: every batch has the sizes that make it an edge of the chain core
(csrc/side/orbx_window_device.h), and a plausibly wrong implementation would give other rows.  The compiled oracle and the two Python
models agree on the new inputs at the small shapes."""
import numpy as np
import pytest

from orb_slam3_modified_amd._window import LDS_MAX, lds_bytes
from tests import localmatch_model as lm
from tests import window_edge_cases as wc


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))


def _only(s, b):
    """The scene with item b alone."""
    t = dict(s)
    for key in ("frame", "pts", "npts", "kp_obs"):
        t[key] = s[key][b:b + 1]
    t["bad"] = {0: s["bad"][b]} if b in s["bad"] else {}
    return t


# ---- batch 1
@pytest.fixture(scope="module")
def pool():
    return wc.many_items_pool()


def test_many_items_sizes_and_the_two_references(pool):
    s = pool
    assert wc.MANY == 2 * 1024 + 5 and s["cap"] == 64 and s["mcap"] == 32 and len(s["frame"]) == wc.P == 13
    assert 1024 % wc.P == 10 and 256 % wc.P == 9                 # the items a workgroup meets in succession differ on both paths
    kind = {k: b for b, k in enumerate(wc.KIND)}
    FA = int(s["frame"][kind["every"]])
    assert s["counts"][FA, 0] == s["cap"] and (s["kp_obs"][kind["allhidden"]] > 0).all() and (s["kp_obs"][kind["every"]] == -1).all()
    assert s["npts"][kind["pairs"]] == s["mcap"] and s["npts"][kind["two"]] == 2 and s["npts"][kind["nopoints"]] == 0
    assert s["counts"][s["frame"][kind["emptyframe"]], 0] == 0 and s["npts"][kind["emptyframe"]] > 0
    assert s["bad"] == {kind["badoctave"]: "octave", kind["badframe"]: "frame"}
    F3 = int(s["frame"][kind["three"]])
    assert s["counts"][F3, 0] == 6 and sum(len(c) for c in wc.in_grid(s, F3)) == 3
    for ori in (True, False):
        want = wc.want_last(s, ori)
        assert _same(want, wc.model_last(s, ori)), ori            # the oracle and the model agree on the pool
        assert want[0][kind["every"]] == (32 if not ori else want[0][kind["every"]]) and want[0][kind["allhidden"]] == 0
    want = wc.want_local(s)
    assert _same(want, wc.model_local(s))
    assert want[0][kind["every"]] == 32 and (want[1][kind["every"]] >= 0).sum() == 32
    # many acceptances with obs > 0 in the full row, and its pairs' second points fall back
    assert want[0][kind["pairs"]] > 16 and (want[2][kind["pairs"]] > 0).sum() > 16
    for nm in (want[0], wc.want_last(s, False)[0]):
        for b, k in enumerate(wc.KIND):
            # every well-formed entry with points, keypoints and an open keypoint among them matches
            assert (nm[b] > 0) == (k not in ("nopoints", "emptyframe", "badoctave", "allhidden", "badframe")), k
            assert (nm[b] == -1) == (b in s["bad"])


def test_many_items_are_independent_on_the_model(pool):
    """The reference rows of the tiled batch are the pool's rows, tiled: the model computes an item from its own row alone."""
    t = wc.tile(pool, 2 * wc.P + 3)
    idx = np.arange(2 * wc.P + 3) % wc.P
    assert set(t["bad"]) == {b for b in range(len(idx)) if idx[b] in pool["bad"]}
    for got, one in ((wc.model_last(t, True), wc.model_last(pool, True)), (wc.model_local(t), wc.model_local(pool))):
        for g, o in zip(got[:3], one[:3]):
            assert np.array_equal(g, o[idx])


@pytest.mark.parametrize("matcher", ("last", "local"))
@pytest.mark.parametrize("stride", (wc.MAX_BLOCKS, wc.GLOBAL_BLOCKS), ids=("lds", "global"))
def test_a_carried_over_workgroup_would_show(pool, matcher, stride):
    """An implementation that starts item b with the hidden bits item b - stride left (no re-zeroing between a workgroup's items) gives
    other rows for more than half of the workgroups.  (The other carry-over, `res` rows left from the item before, is not modelled.)"""
    s = pool
    want = (lambda **k: wc.want_last(s, False, **k)) if matcher == "last" else (lambda **k: wc.want_local(s, **k))
    base = want()
    n_of = s["counts"][np.clip(s["frame"], 0, s["K"] - 1), 0]
    left = (base[2] > 0) & (np.arange(s["cap"])[None] < n_of[:, None])      # the bits a well-formed item leaves
    for b in s["bad"]:
        left[b] = False                                            # (a malformed item leaves before it touches them)
    carried = s["kp_obs"].copy()
    for t in range(wc.P):
        pred = (t - stride) % wc.P
        carried[t] = np.where(left[pred] & (carried[t] <= 0), 1, carried[t])
    other = want(kp_obs=carried)
    changed = [not (base[0][t] == other[0][t] and np.array_equal(base[1][t], other[1][t])) for t in range(wc.P)]
    groups = sum(any(changed[b % wc.P] for b in range(w + stride, wc.MANY, stride)) for w in range(stride))
    assert groups > stride // 2, (groups, changed)
    # and a malformed item is followed by a well-formed one that matches, in one workgroup
    assert any(b % wc.P in s["bad"] and (b + stride) % wc.P not in s["bad"] and base[0][(b + stride) % wc.P] > 0 for b in range(wc.MANY - stride))


# ---- batch 2
@pytest.fixture(scope="module")
def sort_scene():
    return wc.sort_sizes()


def test_sort_sizes_have_the_stated_counts_and_matches(sort_scene):
    s = sort_scene
    assert s["cap"] == 1030 and wc.SORT_N0 == (0, 1, 2, 3, 511, 512, 513, 1023, 1024, 1025) and (s["npts"] == 40).all()
    last, local = wc.want_last(s, False), wc.want_local(s)
    assert (wc.want_last(s, True)[1] == -2).any()                  # the rotation filter removes some
    for f, n0 in enumerate(wc.SORT_N0):
        cells = wc.in_grid(s, f)
        inside = sorted(i for c in cells for i in c)
        n = int(s["counts"][f, 0])
        assert len(inside) == n0 and n == n0 + (0 if n0 == 1025 else 5)
        outside = sorted(set(range(n)) - set(inside))
        if outside:                                               # between the others by index, a NaN among them
            assert np.isnan(s["kps"][f, outside]["x"]).sum() == 1 and (n0 < 4 or (outside[0] > 0 and outside[-1] < n - 1 and np.diff(outside).min() > 1))
        if n0 > 3:
            order = [i for c in cells for i in c]
            assert order != sorted(order)                         # the cells' order is not the index order: the sort has work to do
        for nm, match, _ in (last, local):
            assert (nm[f] > 0) == (n0 > 0)
            if n0 == 0:
                continue
            assert match[f, inside[0]] >= 0 and match[f, inside[-1]] >= 0          # the lowest and the highest index
            assert len(cells[0]) == (1 if n0 < 3 else 2) and all(match[f, i] >= 0 for i in cells[0])
            if n0 > 1:
                assert len(cells[wc.LAST_CELL]) == (1 if n0 < 4 else 2) and all(match[f, i] >= 0 for i in cells[wc.LAST_CELL])
    t = wc.sort_full()
    assert t["cap"] == t["counts"][0, 0] == 1024 == sum(len(c) for c in wc.in_grid(t, 0)) and wc.want_local(t)[0][0] > 30
    small = _only(s, 3)                                            # the references agree where the model is affordable: n0 == 3 ...
    assert _same(wc.want_last(small, True), wc.model_last(small, True)) and _same(wc.want_local(small), wc.model_local(small))
    mid = _only(s, 4)                                              # ... and 511
    assert _same(wc.want_local(mid), wc.model_local(mid))


# ---- batch 3
def test_point_counts_chain_across_64_and_512():
    s = wc.point_counts()
    assert s["mcap"] == 1100 and s["cap"] == 128 and tuple(s["npts"]) == (1, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 1100)
    assert any((m + 1) % 512 == 0 for m in s["npts"]) and any((m + 1) % 512 == 1 for m in s["npts"])   # nlast + 1 on both sides of 512
    full = _only(s, len(s["npts"]) - 1)
    chain, free = wc.model_local(full), wc.model_local(full, chain=False)
    assert _same(chain, wc.want_local(full))
    last = wc.model_last(full, True)
    assert _same(last, wc.want_last(full, True)) and (last[4][0] >= 0).sum() > 512    # more than 512 entries in the histogram
    for taken, alone in ((chain[3][0], free[3][0]), (last[3][0], None)):
        for q in (63, 511, 1023):
            kp = wc.count_target(q)
            assert wc.count_target(q + 1) == kp and full["pts"][0, q]["obs"] > 0
            assert taken[q] == kp and taken[q + 1] != kp                             # the suitor behind the boundary is refused
            assert alone is not None or taken[q + 1] >= 0                             # (the one-key matcher's falls back to a neighbour)
            assert alone is None or alone[q + 1] == kp                                # ... and would have had it without the chain
    # a keypoint taken with obs == 0 is rebound by the next suitor
    q = next(q for q in range(1, 1100, 2) if full["pts"][0, q]["obs"] == 0 and chain[3][0][q] == wc.count_target(q))
    assert chain[3][0][q + 1] == chain[3][0][q]


# ---- batch 4 and 5 (a)
@pytest.fixture(scope="module")
def lanes():
    return wc.list_lanes()


def test_list_lengths_and_positions(lanes):
    s = lanes
    assert s["cap"] == 132 and (s["counts"][:3, 0] == 132).all()
    for f in range(3):
        assert sum(len(c) for c in wc.in_grid(s, f)) == len(wc.in_grid(s, f)[30 * 48 + 20]) == 132      # one cell: walk order == index order
    local, last = wc.want_local(s), wc.want_last(s, False)
    assert _same(local, wc.model_local(s)) and _same(last, wc.model_last(s, False)) and _same(wc.want_last(s, True), wc.model_last(s, True))
    taken_local, taken_last = wc.model_local(s)[3], wc.model_last(s, False)[3]
    for v in (wc.V_LAST, wc.V_SAME_LANE, wc.V_OTHER_LANE):
        lists = wc.lists_of(s, v)
        assert tuple(len(c) for c in lists) == wc.LENGTHS == (63, 64, 65, 128, 129)
        for q, c in enumerate(lists):
            assert [i for i, _, _ in c] == list(range(len(c)))
            ranked = sorted(range(len(c)), key=lambda j: (c[j][1], j))
            if v == wc.V_LAST:                                    # the best is the last entry; the second, before it, of another octave
                assert ranked[0] == len(c) - 1 and ranked[1] == len(c) - 2 and c[-1][2] != c[-2][2] and c[-1][1] <= lm.TH_HIGH
                assert taken_local[v, q] == taken_last[v, q] == len(c) - 1
                continue
            best = 0 if v == wc.V_SAME_LANE else 1
            assert ranked[0] == best and c[best][1] == wc.BEST and taken_last[v, q] == best
            if len(c) <= 64:                                      # the second is the 60 at position 10: accepted
                assert ranked[1] == 10 and c[10][1] == wc.THIRD and taken_local[v, q] == best
            else:                                                 # the true second, 44 at position 64: refused; with the third in its place, accepted
                assert ranked[1] == 64 and ranked[2] == 10 and c[64][1] == wc.SECOND and taken_local[v, q] == -1
                assert (ranked[0] % 64 == ranked[1] % 64) == (v == wc.V_SAME_LANE)
                assert lm.decide(c[:64] + c[65:], s["kp_obs"][v], wc.NN_RATIO) == best
            assert all(o == 0 for _, _, o in c)
    # the distances
    a, b = (c for c in wc.lists_of(s, wc.I_DIST) if len(c) == 2), None
    (first, second), = a
    assert first[1] == 256 and second[1] == 30 and first[2] == second[2] and second[0] == s["kp_dist"]["second_256"]
    for nm, match, _ in (local, last):
        assert nm[wc.I_DIST] == 2 and match[wc.I_DIST, s["kp_dist"]["second_256"]] == 0 and match[wc.I_DIST, s["kp_dist"]["best_100"]] == 1
        assert match[wc.I_DIST, s["kp_dist"]["best_101"]] == -1
    assert [c[0][1] for c in wc.lists_of(s, wc.I_DIST)[1:]] == [100, 101]


def test_chunk_item_sums_to_the_room_and_one_more(lanes):
    s = lanes
    lengths = [len(c) for c in wc.lists_of(s, wc.I_CHUNK)]
    cap, mcap = s["cap"], s["mcap"]
    assert tuple(lengths) == wc.CHUNK_LISTS and lengths[0] == cap and lengths[1] + lengths[2] == cap and lengths[3] + lengths[4] == cap + 1
    limit = wc.room_limit(cap, mcap, cap)
    assert limit == lds_bytes(cap, mcap) + 4 * cap and limit % 16 == 0
    assert wc.plan_room(limit, cap, mcap) == cap and wc.plan_room(limit - 16, cap, mcap) is None and wc.plan_room(LDS_MAX, cap, mcap) > sum(lengths)
    assert wc.chunk_cuts(lengths, cap) == [0, 1, 3, 4] and wc.chunk_cuts(lengths, cap + 1) == [0, 1, 3] and wc.chunk_cuts(lengths, 10 ** 6) == [0]
    # what a chunk leaves hidden reaches the next: the second 66 loses keypoint 65 to the first
    taken = wc.model_local(s)[3][wc.I_CHUNK]
    assert list(taken[:5]) == [131, 65, 64, 63, 66] and list(wc.model_last(s, False)[3][wc.I_CHUNK][:5]) == [131, 65, 64, 63, 66]


# ---- batch 5 (b)
def test_global_cut_falls_at_the_room():
    s = wc.global_cut()
    assert s["cap"] == 64 and (s["npts"] == 1100).all()
    for b, per, cut in ((0, 64, 1024), (1, 63, 1040)):
        p = s["pts"][b]
        assert len({(float(x), float(y), int(l)) for x, y, l in zip(p["x"], p["y"], p["level"])}) == 1      # every point has the first one's window
        assert len(wc.lists_of(_only(s, b), 0)[0]) == per
        lengths = [per] * 1100
        assert sum(lengths) > wc.GLOBAL_ROOM == 65536 and wc.chunk_cuts(lengths, wc.GLOBAL_ROOM) == [0, cut]
        assert (cut * per == wc.GLOBAL_ROOM) == (b == 0)         # the cut exactly at the room, resp. with a remainder
    for want in (wc.want_local(s), wc.want_last(s, False)):
        assert (want[0] > 60).all() and (want[1] >= 1040).any(1).all()      # points of the second chunk bind too


# ---- batch 6
def test_default_limit_switch():
    c = wc.largest_lds_capacity()
    assert c == 2470
    assert lds_bytes(c, 64) + 4 * c <= LDS_MAX < lds_bytes(c + 1, 64) + 4 * (c + 1)
    assert wc.plan_room(LDS_MAX, c, 64) == (LDS_MAX - lds_bytes(c, 64)) // 4 >= c and wc.plan_room(LDS_MAX, c + 1, 64) is None
    for cap in (c, c + 1):
        s = wc.limit_switch(cap)
        assert s["cap"] == s["counts"][0, 0] == cap and s["npts"][0] == 60 and s["mcap"] == 64
        for nm, match, _ in (wc.want_local(s), wc.want_last(s, False)):
            assert nm[0] > 50 and match[0, 0] >= 0 and match[0, cap - 1] >= 0


# ---- batch 7
def test_capacity_max():
    s = wc.capacity_max()
    n = 32768
    assert s["cap"] == n == s["counts"][0, 0] and s["pts"].shape == (2, 100)
    k = s["kps"][0]
    cell = np.round(k["x"] / 10.0).astype(int) * 48 + np.round(k["y"] / 10.0).astype(int)
    assert np.round(k["x"] / 10.0).max() == 63 and np.round(k["y"] / 10.0).max() == 47 and k["x"].min() > 0 and k["y"].min() > 0   # all in the grid
    assert (np.diff(cell) < 0).any()                              # not in the cells' order by index
    p = s["pts"][0]
    per_window = [int(((np.abs(k["x"] - x) < 20) & (np.abs(k["y"] - y) < 20)).sum()) for x, y in zip(p["x"], p["y"])]
    assert max(per_window) > 64
    for nm, match, obs in (wc.want_local(s), wc.want_last(s, False)):
        assert match[1, n - 1] == 2 and match[1, n - 2] == 1 and match[1, 0] == 0 and match[0, 0] == 0      # index 32767 matched
        assert match[0, n - 1] == -1 and obs[0, n - 1] == 3     # hidden in item 0: the point goes elsewhere
        differ = np.nonzero(match[0] != match[1])[0]
        assert n - 1 in differ and len(differ) <= 2 and nm[0] >= nm[1] - 1
    assert np.array_equal(s["kp_obs"][0, :n - 1], s["kp_obs"][1, :n - 1]) and np.array_equal(s["pts"][0], s["pts"][1])


# ---- the model-checked matchers at the reduced sizes
def test_proj_and_rig_pool_and_sizes(pool):
    r = wc.rig_of(pool, cap_r=60)
    assert r["cap_l"] == 64 and r["cap_r"] == 60 and (r["counts_r"][:, 0] <= r["counts"][:, 0]).all()
    rows = [wc.model_proj(pool, False), wc.model_rig(r, "local"), wc.model_rig(r, "last", False)]
    for nm, *_ in rows:
        for b, k in enumerate(wc.KIND):
            assert (nm[b] > 0) == (k not in ("nopoints", "emptyframe", "badoctave", "allhidden", "badframe")), k
            assert (nm[b] == -1) == (b in pool["bad"])
    t = wc.tile(r, 2 * wc.P + 3)                                   # independent on the rig's model too
    idx = np.arange(2 * wc.P + 3) % wc.P
    for g, o in zip(wc.model_rig(t, "local")[:3], rows[1][:3]):
        assert np.array_equal(g, o[idx])
    s = wc.sort_sizes(wc.PROJ_SORT_N0)
    r = wc.rig_of(s)
    assert [sum(len(c) for c in wc.in_grid(s, f)) for f in range(s["K"])] == list(wc.PROJ_SORT_N0) == [0, 1, 2, 3, 63, 64, 65, 513]
    right = [sum(len(c) for c in lm.assign_grid(r["kps_r"][f, :r["counts_r"][f, 0]], r["bounds"][f])) for f in range(s["K"])]
    assert all(a != b for a, b in zip(right[4:], wc.PROJ_SORT_N0[4:])) and right[-1] > 300 and right[0] == 0     # other counts on the second camera
    for nm in (wc.model_proj(s, True)[0], wc.model_rig(r, "local")[0], wc.model_rig(r, "last")[0]):
        assert nm[0] == 0 and (nm[1:] > 0).all()
    s = wc.point_counts(wc.PROJ_NLAST)
    assert tuple(s["npts"]) == (64, 65, 513)
    bound = wc.model_proj(s, True)[2]
    # (every bind of this matcher takes its keypoint: the 128 are gone before point 511, where the edge is the scan's and the loops')
    assert bound[1, 63] == wc.count_target(63) == wc.count_target(64) != bound[1, 64] and (bound[2, 400:] == -1).all() and (bound[2] >= 0).sum() > 64
    rl = wc.model_rig(wc.rig_of(s), "last", False)[3][2]["points"]
    assert rl[511]["left"] == ("accept", wc.count_target(511)) and rl[512]["left"] != rl[511]["left"]


def test_proj_and_rig_list_lengths():
    s = wc.lanes_plain()
    assert tuple(s["counts"][:15, 0]) == wc.LENGTHS * 3
    bound = wc.model_proj(s, False)[2][:, 0]
    r = wc.rig_of(s, drop=lambda n: 0)
    nm, match, _, trace = wc.model_rig(r, "local")
    last = wc.model_rig(r, "last", False)
    for v in wc.PLAIN_VARIANTS:
        for k, length in enumerate(wc.LENGTHS):
            b = 5 * v + k
            assert trace[b][0]["lists"][0] == length and trace[b][0]["lists"][1] in (0, length)
            best = length - 1 if v == wc.V_LAST else 0 if v == wc.V_SAME_LANE else 1
            assert bound[b] == best and last[1][b, best] == 0 and last[1][b, r["cap_l"] + length - 1 - best] == 0
            if v == wc.V_LAST or length <= 64:
                assert trace[b][0]["left"][:2] == ("accept", best) and trace[b][0]["right"][0] == "accept"     # (the partner slot may be the left's)
            else:                                                 # the true second, 44 at position 64, refuses; the :126 exit skips the right camera
                assert trace[b][0]["left"] == "ratio" and trace[b][0]["right"] is None and nm[b] == 0
    d = s["kp_dist"]
    sites = wc.model_proj(s, False)[2][15]
    assert sites[0] == d["second_256"] and sites[1] == d["best_100"] and sites[2] == -1 and nm[15] >= 2 and match[15, d["best_101"]] == -1


def test_rig_switch_and_capacity():
    from orb_slam3_modified_amd._window import rig_lds_bytes
    c, q = wc.largest_rig_lds_capacity(wc.RIG_SWITCH_MCAP), wc.RIG_SWITCH_MCAP
    assert rig_lds_bytes(c, c, q) + 8 * c <= LDS_MAX < rig_lds_bytes(c + 1, c + 1, q) + 8 * (c + 1)
    r = wc.rig_capacity_max()
    assert r["cap_l"] == r["cap_r"] == r["counts"][0, 0] == r["counts_r"][0, 0] == 16384 and r["kp_obs"][0, 32767] == 3 and (r["kp_obs"][1] == -1).all()
    for entry in ("local", "last"):
        nm, match, obs, _ = wc.model_rig(r, entry, False)
        assert match[1, 32767] == 0 and match[0, 32767] == -1 and obs[0, 32767] == 3 and match[0, 0] == match[1, 0] == 0
