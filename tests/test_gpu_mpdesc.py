"""The batched ComputeDistinctiveDescriptors (liborbx_mpdesc.so, orb_slam3_modified_amd/mpdesc.py) on the GPU: best, median and the whole
output table equal tests/mpdesc_model.py's -- on the constructed batch of tests/mpdesc_cases.py through the host form, on the buffers a
batch extraction left in HBM through the device form, chained into the batched Fuse search, and under every routing of the size classes.
Everything is exact equality."""
import ctypes as C

import numpy as np
import pytest

from orb_slam3_modified_amd import ORBextractor, _lib
from orb_slam3_modified_amd.fuse import FuseBatch, FuseSide, grid_parameters
from orb_slam3_modified_amd.mpdesc import MID_CAP, MID_MAX, OBS_DTYPE, SMALL_CAP, SMALL_MAX, DistinctBatch, DistinctSide
from tests import fuse_cases as fc
from tests import fuse_model as fm
from tests import mpdesc_cases as mc
from tests import mpdesc_model as mm
from tests import trimatch_cases as tc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests.pair_batch_util import Batch as HbmBatch, dev  # noqa: E402


def _check(got, want, where):
    """best [M], median [M] and the whole table [R, 32]."""
    for g, w, name in zip(got, want, ("best", "median", "table")):
        g = np.asarray(g)
        assert g.shape == w.shape, (where, name, g.shape, w.shape)
        bad = np.nonzero(np.asarray(g != w).reshape(len(w), -1).any(1))[0]
        assert len(bad) == 0, (where, name, bad[:5].tolist(), g[bad[:5]].tolist(), w[bad[:5]].tolist())


@pytest.fixture(scope="module")
def case():
    """The constructed batch and -- computed once -- the model's results with and without out_rows."""
    c = mc.build()
    M = len(c["obs_start"]) - 1
    c["want", True] = mm.select(c["desc"], c["counts"], c["obs"], c["obs_start"], c["out_rows"], mc.sentinel_table(c["table_rows"]))
    c["want", False] = mm.select(c["desc"], c["counts"], c["obs"], c["obs_start"], None, mc.sentinel_table(M))
    c["side"] = DistinctSide(c["desc"], c["counts"], mc.K, mc.CAP)
    c["M"] = M
    return c


def _host(db, c, with_rows):
    table = mc.sentinel_table(c["table_rows"] if with_rows else c["M"])
    r = db.select(c["side"], c["obs"], c["obs_start"], c["out_rows"] if with_rows else None, table)
    assert r.desc is table
    return r.best, r.median, r.desc


# ---- test 1: the constructed batch through the host form
def test_constructed_batch_through_the_host_form(case):
    c = case
    db = DistinctBatch(0)
    for with_rows in (True, False):
        got = _host(db, c, with_rows)
        _check(got, c["want", with_rows], ("host", with_rows))
    best, median, table = got
    P = mc.PLANTED
    assert best[P["even_middles"]] == 0 and best[P["later_tie"]] == 1 and median[P["complement"]] == 3 and best[P["empty"]] == -1
    for name in mc.expected_malformed():
        if not name.startswith("out_row"):
            assert best[P[name]] == -2 and median[P[name]] == -1 and (table[P[name]] == mc.SENTINEL).all(), name
    # a table of the caller's is optional: M zeroed rows
    r = db.select(c["side"], c["obs"], c["obs_start"])
    want = mm.select(c["desc"], c["counts"], c["obs"], c["obs_start"], None, np.zeros((c["M"], 32), np.uint8))
    _check(r, want, "zeroed")
    db.close()


# ---- test 2: device-resident, on the buffers a batch extraction left in HBM
@pytest.fixture(scope="module")
def hbm():
    ex = ORBextractor(*tc.EXTRACTOR, device_id=0)
    bt = HbmBatch(ex, tc.frames())
    B, cap = bt.B, bt.cap
    assert (bt.hc[:, 0] > 250).all()
    M = 3 * cap
    obs, obs_start = mc.random_observations(bt.hc, M, 1130)
    rows = np.random.default_rng(3).permutation(M + 11)[:M].astype(np.int32)
    want = mm.select(bt.hd, bt.hc, obs, obs_start, rows, np.zeros((M + 11, 32), np.uint8))
    assert (want[0] >= -1).all() and (want[0] > 0).sum() > M // 2
    t = lambda a: torch.from_numpy(a).to(dev())   # noqa: E731
    return dict(bt=bt, M=M, obs=obs, obs_start=obs_start, rows=rows, want=want, tobs=t(obs.view(np.int32).reshape(-1, 2)), tstart=t(obs_start),
                trows=t(rows), side=DistinctSide(bt.desc, bt.counts, B, cap))


def _device(db, h, stream):
    table = torch.zeros((h["M"] + 11, 32), dtype=torch.uint8, device=dev())
    torch.cuda.synchronize()
    return db.select_device(h["side"], h["tobs"], h["tstart"], h["trows"], table, stream=stream.cuda_stream)


def test_device_form_on_extracted_buffers_two_handles_two_streams(hbm):
    h = hbm
    a, b = DistinctBatch(0), DistinctBatch(0)
    sa, sb = h["bt"].s, torch.cuda.Stream(device=dev())
    ra, rb = _device(a, h, sa), _device(b, h, sb)
    sa.synchronize()
    sb.synchronize()
    got = [tuple(x.cpu().numpy() for x in r) for r in (ra, rb)]
    _check(got[0], h["want"], "stream a")
    for x, y in zip(*got):
        assert x.tobytes() == y.tobytes()
    # a second call on the same handle and the handle's own stream: the scratch is reused
    r = a.select_device(h["side"], h["tobs"], h["tstart"], h["trows"], torch.zeros_like(ra.desc))
    torch.cuda.synchronize()
    _check(tuple(x.cpu().numpy() for x in r), h["want"], "own stream")
    a.close()
    b.close()
    b.close()


# ---- test 3: the table goes on to the batched Fuse search without leaving the device
def test_the_table_is_the_fuse_searchs_pdesc(hbm):
    h, bt = hbm, hbm["bt"]
    B, cap = bt.B, bt.cap
    parm = np.stack([grid_parameters(0, 0, tc.WIDTH, tc.HEIGHT)] * B)
    pl = [(0, 1), (2, 3), (6, 7)]                                # (searched keyframe, the frame the queries come from)
    # point q + p * cap is seen once somewhere and three times in keypoint q of frame g: that keypoint's descriptor wins, as row 1
    rng = np.random.default_rng(1148)
    lists = []
    for _, g in pl:
        for q in range(cap):
            f = int(rng.integers(0, B))
            lists.append([(f, int(rng.integers(0, bt.hc[f, 0])))] + [(g, q)] * 3 if q < bt.hc[g, 0] else [])
    obs = np.array([o for l in lists for o in l], OBS_DTYPE)
    obs_start = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
    model = mm.select(bt.hd, bt.hc, obs, obs_start, h["rows"], np.zeros((h["M"] + 11, 32), np.uint8))
    assert set(model[0].tolist()) <= {-1, 0, 1} and (model[0] == 1).sum() > 2 * cap
    db = DistinctBatch(0)
    table = torch.zeros((h["M"] + 11, 32), dtype=torch.uint8, device=dev())
    torch.cuda.synchronize()
    r = db.select_device(h["side"], torch.from_numpy(obs.view(np.int32).reshape(-1, 2)).to(dev()), torch.from_numpy(obs_start).to(dev()), h["trows"], table,
                         stream=bt.s.cuda_stream)
    rows = [fc.derived_queries(bt.frame(g)[0], cap, 200 + p) for p, (_, g) in enumerate(pl)]
    query, nquery = np.stack([q for q, _ in rows]), np.array([n for _, n in rows], np.int32)
    for p in range(len(pl)):                                     # query q of row p asks for point q + p * cap's row of the table
        live = query[p]["point"] >= 0
        query[p]["point"][live] = h["rows"][np.arange(cap)[live] + p * cap]
    pairs = np.array([k for k, _ in pl], np.int32)
    inv = fc.plain_inv_level_sigma2()
    want = fm.search(bt.hk, bt.hd, bt.hc, None, parm, query, nquery, pairs, model[2], inv, True, 50)
    assert (want[0] >= 0).all() and want[0].sum() > 30          # tests/test_gpu_fuse.py finds some 30 a pair on these frames
    side = FuseSide(bt.kps, bt.desc, bt.counts, torch.from_numpy(parm).to(dev()), B, cap, None)
    fb = FuseBatch(0)
    fb.grids_device(side, stream=bt.s.cuda_stream)
    out = fb.search_device(side, torch.from_numpy(query.view(np.uint8).reshape(len(pl), cap, 32)).to(dev()), torch.from_numpy(nquery).to(dev()),
                           torch.from_numpy(pairs).to(dev()), r.desc, inv, True, 50, stream=bt.s.cuda_stream)
    bt.s.synchronize()
    for g, w, name in zip((out.nfound, out.best_idx, out.best_dist), want, ("nfound", "best_idx", "best_dist")):
        assert np.array_equal(g.cpu().numpy(), w), name
    _check(tuple(x.cpu().numpy() for x in r), model, "chain")
    fb.close()
    db.close()


# ---- test 4: every routing of the size classes gives the same bytes
@pytest.mark.parametrize("small_max,mid_max", ((0, MID_CAP), (0, 0), (8, 32), (SMALL_CAP, SMALL_CAP)))
def test_forced_routing(case, hbm, monkeypatch, small_max, mid_max):
    """(0, 256): the LDS-matrix form on every point it can take; (0, 0): the recomputing form on every point; the default handle of the
    other tests is the lane-per-observation form on every point it can take (64, 256); two more with the boundaries moved."""
    assert (SMALL_MAX, MID_MAX) == (SMALL_CAP, MID_CAP)
    monkeypatch.setenv("ORBX_MPDESC_SMALL_MAX", str(small_max))
    monkeypatch.setenv("ORBX_MPDESC_MID_MAX", str(mid_max))
    db = DistinctBatch(0)
    monkeypatch.delenv("ORBX_MPDESC_SMALL_MAX")
    monkeypatch.delenv("ORBX_MPDESC_MID_MAX")
    c = case
    _check(_host(db, c, True), c["want", True], ("forced", small_max, mid_max))
    r = _device(db, hbm, hbm["bt"].s)
    hbm["bt"].s.synchronize()
    _check(tuple(x.cpu().numpy() for x in r), hbm["want"], ("forced hbm", small_max, mid_max))
    db.close()


# ---- test 5: what the host can check
def test_host_checked_errors(hbm):
    h = hbm
    M = h["M"]
    L = _lib.mpdesc_lib()
    db = DistinctBatch(0)
    sd = h["side"]._struct()
    p_ = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    sentinel = 77
    table = torch.full((M + 11, 32), sentinel, dtype=torch.uint8, device=dev())
    best, median = torch.full((M,), sentinel, dtype=torch.int32, device=dev()), torch.full((M,), sentinel, dtype=torch.int32, device=dev())
    ok = [C.byref(sd), p_(h["tobs"]), len(h["obs"]), p_(h["tstart"]), M, p_(h["trows"]), p_(table), M + 11, p_(best), p_(median), None]
    for idx, v in ((0, None), (1, None), (2, 0), (3, None), (4, 0), (6, None), (7, 0), (7, -3), (8, None), (9, None),
                   (6, C.c_void_p(table.data_ptr() + 8))):
        a_ = list(ok)
        a_[idx] = v
        assert L.orbx_mpdesc_select_device(db._h, *a_) == _lib.ORBX_E_INVALID, (idx, v)
        assert len(L.orbx_mpdesc_last_error(db._h)) > 10
    for field, v in (("d_desc", None), ("d_counts", None), ("nframes", 0), ("capacity", 0), ("capacity", 2 ** 30)):
        sb = h["side"]._struct()
        setattr(sb, field, v)
        assert L.orbx_mpdesc_select_device(db._h, C.byref(sb), *ok[1:]) == _lib.ORBX_E_INVALID, field
    if torch.cuda.device_count() > 1:                            # a foreign device
        far = torch.zeros(M, dtype=torch.int32, device=torch.device("cuda", 1))
        a_ = list(ok)
        a_[8] = p_(far)
        assert L.orbx_mpdesc_select_device(db._h, *a_) == _lib.ORBX_E_INVALID
        assert b"device" in L.orbx_mpdesc_last_error(db._h)
    torch.cuda.synchronize()
    # nothing was launched: no result, no row was written
    assert (table == sentinel).all() and (best == sentinel).all() and (median == sentinel).all()
    host = np.zeros((4, 32), np.uint8)
    with pytest.raises(_lib.OrbxError):
        db.select(DistinctSide(h["bt"].hd, h["bt"].hc, h["bt"].B, h["bt"].cap), np.zeros(0, OBS_DTYPE), np.zeros(5, np.int32), None, host)
    with pytest.raises(ValueError):
        db.select(DistinctSide(h["bt"].hd, h["bt"].hc, h["bt"].B, h["bt"].cap), h["obs"], h["obs_start"], h["rows"])
    assert L.orbx_mpdesc_select_device(db._h, *ok) == 0         # and the handle still works
    torch.cuda.synchronize()
    _check((best.cpu().numpy(), median.cpu().numpy()), h["want"][:2], "after the errors")
    db.close()
