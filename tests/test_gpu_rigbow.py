"""liborbx_rigbow.so (orb_slam3_modified_amd/rigbow.py) on the GPU: every output word of the rig SearchByBoW equals tests/rigbow_model.py on
the constructed batch of tests/rigbow_cases.py, on every path and in both modes; the stacker equals the model; single-camera frames give
MatchBatch's bytes; and one device-resident chain from a FisheyeBatch extraction through the stacker and BowBatch to the matches."""
import ctypes as C

import numpy as np
import pytest

from orb_slam3_modified_amd import ORBextractor, ORBVocabulary, OrbxError, _lib, synth
from orb_slam3_modified_amd._lib import KP_DTYPE
from orb_slam3_modified_amd.rigbow import FRAME, KEYFRAMES, LDS_MAX, RigBowBatch, RigBowSide, lds_bytes
from tests import match_batch_cases as mc
from tests import rigbow_cases as rc
from tests import rigbow_model as rm
from tests import trimatch_cases as tc
from tests.vocab_util import make_vocabulary

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

COMBOS = [(mode, valid, ori) for mode in (FRAME, KEYFRAMES) for valid in (True, False) for ori in (True, False)]
PATHS = {"default": {}, "global": {"ORBX_RIGBOW_LDS": "0"}, "trips": {"ORBX_RIGBOW_WAVE_NODE": "0"},
         "global trips": {"ORBX_RIGBOW_LDS": "0", "ORBX_RIGBOW_WAVE_NODE": "0"}}


def _dev():
    return torch.device("cuda", 0)


def _handle(monkeypatch, env):
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    rb = RigBowBatch(0)
    for k_ in env:
        monkeypatch.delenv(k_)
    return rb


@pytest.fixture(scope="module")
def constructed():
    """The batch and -- computed once -- the model's whole rows (nmatches, b2a, a2b) of both pair lists under every run, mode, valid form
    and check_orientation.  A malformed pair: -1 and rows of -1."""
    c = rc.build()
    for which, pairs, bad in (("pairs", rc.PAIRS, {}), ("bad_pairs", rc.BAD_PAIRS, rc.MALFORMED)):
        P = len(pairs)
        for run, ratio in rc.RUNS.items():
            for mode, valid, ori in COMBOS:
                n, b2a, a2b = np.full(P, -1, np.int32), np.full((P, rc.CAP), -1, np.int32), np.full((P, rc.CAP, 2), -1, np.int32)
                for p, (ia, ib) in enumerate(pairs.tolist()):
                    if p in bad:
                        continue
                    (da, aa, va, fa, nla), (db, ab, vb, fb, nlb) = rc.frame(c, ia), rc.frame(c, ib)
                    n[p], row, inv = rm.search_by_bow(da, aa, va if valid else None, fa, nla, db, ab, vb if valid else None, fb, nlb, mode, ratio, ori)
                    b2a[p, :len(db)], a2b[p, :len(da)] = row, inv
                c["want", which, run, mode, valid, ori] = (n, b2a, a2b)
    return c


def _side(c, valid, nleft=True):
    return RigBowSide(c["kps"], c["desc"], c["counts"], c["fv_node"], c["fv_ptr"], c["fv_feat"], c["fv_n"], len(c["counts"]), c["desc"].shape[1],
                      c["valid"] if valid else None, c["nleft"] if nleft else None)


@pytest.mark.parametrize("path", list(PATHS))
def test_constructed_batch_on_every_path(constructed, monkeypatch, path):
    """Both modes, both forms of `valid`, with and without check_orientation, both nn_ratios, the planted pairs and the malformed ones,
    through the host form.  "trips" and "global trips" put every node through the trip loop."""
    c = constructed
    assert lds_bytes(rc.CAP, rc.CAP) <= LDS_MAX
    rb = _handle(monkeypatch, PATHS[path])
    for run, ratio in rc.RUNS.items():
        for mode, valid, ori in COMBOS:
            side = _side(c, valid)
            for which, pairs in (("pairs", rc.PAIRS), ("bad_pairs", rc.BAD_PAIRS)):
                r = rb.bow_pairs(side, side, pairs, mode, ratio, ori)
                for g, w, name in zip((r.nmatches, r.b2a, r.a2b), c["want", which, run, mode, valid, ori], ("nmatches", "b2a", "a2b")):
                    bad = np.nonzero((g != w).reshape(len(w), -1).any(1))[0]
                    assert len(bad) == 0, (path, which, run, mode, valid, ori, name, bad.tolist())
                if which == "bad_pairs":
                    for p in rc.MALFORMED:
                        assert r.nmatches[p] == -1 and (r.b2a[p] == -1).all() and (r.a2b[p] == -1).all(), p
                    assert r.nmatches[0] > 0 and r.nmatches[7] > 0
                    continue
                for name, (p, crun, want) in rc.CLAIMS.items():           # the named outcomes, read off the kernel's rows
                    if crun == run:
                        wl, wr = want(mode, valid, ori)
                        held = tuple(int(v) for v in r.a2b[p, rc.PLANTED[name]])
                        assert held == (-1 if wl is None else rc.KP[wl], -1 if wr is None else rc.KP[wr]), (path, name, mode, valid, ori)
    rb.close()


def test_either_output_alone_and_rejected_arguments(constructed):
    c = constructed
    rb = RigBowBatch(0)
    side = _side(c, True)
    full = rb.bow_pairs(side, side, rc.PAIRS, FRAME, rc.RATIO, True)
    M, hs = _lib.rigbow_lib(), side._host()
    s = hs._struct()
    P = len(rc.PAIRS)
    n, b2a, a2b = np.zeros(P, np.int32), np.zeros((P, rc.CAP), np.int32), np.zeros((P, rc.CAP, 2), np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    pairs = np.ascontiguousarray(rc.PAIRS)
    assert M.orbx_rigbow_pairs(rb._h, C.byref(s), C.byref(s), p(pairs), P, FRAME, rc.RATIO, 1, p(b2a), None, p(n)) == 0
    assert np.array_equal(b2a, full.b2a) and np.array_equal(n, full.nmatches)
    assert M.orbx_rigbow_pairs(rb._h, C.byref(s), C.byref(s), p(pairs), P, FRAME, rc.RATIO, 1, None, p(a2b), p(n)) == 0
    assert np.array_equal(a2b, full.a2b) and np.array_equal(n, full.nmatches)
    assert M.orbx_rigbow_pairs(rb._h, C.byref(s), C.byref(s), p(pairs), P, FRAME, rc.RATIO, 1, None, None, p(n)) == _lib.ORBX_E_INVALID
    assert len(M.orbx_rigbow_last_error(rb._h)) > 10
    with pytest.raises(OrbxError):
        rb.bow_pairs(side, side, rc.PAIRS, 5, 0.7, True)
    rb.close()
    rb.close()


def test_the_stacker_equals_the_model():
    kl, dl, cl, kr, dr, cr = rc.rig_frames()
    want = rm.stack(kl, dl, cl, kr, dr, cr, rc.CAP_S)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], a.shape[1], -1) if a.dtype == KP_DTYPE   # noqa: E731
                                    else np.ascontiguousarray(a)).to(_dev())
    rb = RigBowBatch(0)
    s = torch.cuda.Stream(device=_dev())
    torch.cuda.synchronize()
    out = rb.stack_device(to(kl), to(dl), to(cl), to(kr), to(dr), to(cr), cap_s=rc.CAP_S, stream=s.cuda_stream)
    s.synchronize()
    assert out.kps.cpu().numpy().tobytes() == want[0].tobytes()
    assert np.array_equal(out.desc.cpu().numpy(), want[1])
    assert np.array_equal(out.counts.cpu().numpy(), want[2]) and np.array_equal(out.nleft.cpu().numpy(), want[3])
    assert sorted(np.nonzero(want[3] < 0)[0].tolist()) == sorted(rc.RIG_MALFORMED)
    M = _lib.rigbow_lib()
    assert M.orbx_rigbow_stack_device(rb._h, None, rc.CAP_S, None, None, None, None, None) == _lib.ORBX_E_INVALID
    rb.close()


@pytest.mark.parametrize("mode", [FRAME, KEYFRAMES])
def test_single_camera_frames_equal_match_batch(monkeypatch, mode):
    """nleft = -1 everywhere (as an array and as NULL): the bytes of MatchBatch on the same arrays, tests/match_batch_cases.py's batch in
    two calls.  k_rigbow_pairs is k_match_pairs' text with a second camera: this holds on each of the four paths (LDS or global,
    register path or trip loop), both handles created on the same one."""
    from orb_slam3_modified_amd.match import MatchBatch, MatchSide
    c = mc.build()
    c["nleft"] = np.full(mc.K, -1, np.int32)
    for path, env in PATHS.items():
        menv = {k_.replace("ORBX_RIGBOW_", "ORBX_MATCH_"): v_ for k_, v_ in env.items()}
        for k_, v_ in menv.items():
            monkeypatch.setenv(k_, v_)
        mb = MatchBatch(0)
        for k_ in menv:
            monkeypatch.delenv(k_)
        rb = _handle(monkeypatch, env)
        for valid in (True, False):
            ms = MatchSide(c["kps"], c["desc"], c["counts"], c["fv_node"], c["fv_ptr"], c["fv_feat"], c["fv_n"], mc.K, mc.CAP, c["valid"] if valid else None)
            for pairs in (mc.PAIRS[:8], mc.PAIRS[8:]):
                w = mb.bow_pairs(ms, ms, pairs, mode, mc.RATIO, True)
                for nleft in (True, False):
                    r = rb.bow_pairs(_side(c, valid, nleft), _side(c, valid, nleft), pairs, mode, mc.RATIO, True)
                    assert np.array_equal(r.nmatches, w.nmatches) and np.array_equal(r.b2a, w.b2a), (path, mode, valid, nleft)
                    assert np.array_equal(r.a2b[:, :, 0], w.a2b) and (r.a2b[:, :, 1] == -1).all(), (path, mode, valid, nleft)
                assert (w.nmatches > 0).any()
        mb.close()
        rb.close()


def test_device_resident_chain(tmp_path):
    """FisheyeBatch extraction -> stack_device -> BowBatch.transform_device on the stacked buffers -> bow_pairs_device, a keyframe rig
    against a frame rig; nothing leaves the device in between, and the results equal the model on the downloaded stacked frames."""
    from orb_slam3_modified_amd.bow import BowBatch
    from orb_slam3_modified_amd.fisheye import FisheyeBatch
    exL = ORBextractor(*tc.EXTRACTOR, device_id=0)
    exR = exL.clone()
    left = synth.make_stream(4, 256, 256)
    right = np.ascontiguousarray(np.roll(left, -24, axis=2))
    B, cap, dev = 4, exL.capacity, _dev()
    z = lambda *shape, dt=torch.uint8: torch.zeros(shape, dtype=dt, device=dev)   # noqa: E731
    kL, dL, cL, kR, dR, cR = z(B, cap, 28), z(B, cap, 32), z(B, 2, dt=torch.int32), z(B, cap, 28), z(B, cap, 32), z(B, 2, dt=torch.int32)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    fb = FisheyeBatch(exL, exR)
    iL, iR = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
    fb.extract_device(iL, iR, (80, 256), (0, 176), kL, dL, cL, kR, dR, cR, stream=s.cuda_stream)
    s.synchronize()
    hdl, hcl, hdr, hcr = dL.cpu().numpy(), cL.cpu().numpy(), dR.cpu().numpy(), cR.cpu().numpy()
    assert (hcl[:, 0] > 50).all() and (hcr[:, 0] > 50).all()
    voc = str(tmp_path / "voc.txt")
    make_vocabulary(voc, np.concatenate([hdl[f, :hcl[f, 0]] for f in range(B)]), 10, 3, seed=28)
    gv = ORBVocabulary(exL)
    assert gv.loadFromTextFile(voc)
    rb, bb = RigBowBatch(0), BowBatch(gv, 2)
    cap_s = 2 * cap
    st = rb.stack_device(kL, dL, cL, kR, dR, cR, stream=s.cuda_stream)
    fv = bb.transform_device(st.desc, st.counts, B, cap_s, stream=s.cuda_stream, bow=False)
    side = RigBowSide.of(st, fv)
    pairs = np.array([(0, 1), (1, 2), (2, 3), (3, 0)], np.int32)
    out = {mode: rb.bow_pairs_device(side, side, torch.from_numpy(pairs).to(dev), mode, 0.7, True, stream=s.cuda_stream) for mode in (FRAME, KEYFRAMES)}
    s.synchronize()
    # the stacked frames are the model's on the downloaded extraction
    hk = lambda t: t.cpu().numpy().view(KP_DTYPE).reshape(B, -1)   # noqa: E731
    want = rm.stack(hk(kL), hdl, hcl, hk(kR), hdr, hcr, cap_s)
    sk, sd, sc, snl = hk(st.kps), st.desc.cpu().numpy(), st.counts.cpu().numpy(), st.nleft.cpu().numpy()
    assert sk.tobytes() == want[0].tobytes() and np.array_equal(sd, want[1]) and np.array_equal(sc, want[2]) and np.array_equal(snl, want[3])
    assert np.array_equal(snl, hcl[:, 0]) and st.capacity == cap_s
    hfv = [f[1] for f in fv_frames(fv, B)]
    assert all(max(max(l) for l in d.values()) >= snl[f] for f, d in enumerate(hfv))      # right features carry nleft + j
    two = 0
    for mode in (FRAME, KEYFRAMES):
        n, b2a, a2b = out[mode].nmatches.cpu().numpy(), out[mode].b2a.cpu().numpy(), out[mode].a2b.cpu().numpy()
        for i, (ia, ib) in enumerate(pairs.tolist()):
            na, nb = int(sc[ia, 0]), int(sc[ib, 0])
            wn, wb2a, wa2b = rm.search_by_bow(sd[ia, :na], sk[ia, :na]["angle"], None, hfv[ia], int(snl[ia]), sd[ib, :nb], sk[ib, :nb]["angle"], None,
                                              hfv[ib], int(snl[ib]), mode, 0.7, True)
            assert n[i] == wn and np.array_equal(b2a[i, :nb], wb2a) and (b2a[i, nb:] == -1).all(), (mode, i)
            assert np.array_equal(a2b[i, :na], wa2b) and (a2b[i, na:] == -1).all(), (mode, i)
            if mode == FRAME:
                two += int(((wa2b >= 0).sum(1) == 2).sum())
        assert (n > 10).all(), n
    assert two > 0                                       # some keyframe feature holds a left and a right slot
    for h in (rb, bb, fb):
        h.close()


def _device_side(s, with_valid):
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (-1,)) if a.dtype.names else np.ascontiguousarray(a)).to(_dev())   # noqa: E731
    t = {k: to(s[k]) for k in ("kps", "desc", "counts", "fv_node", "fv_ptr", "fv_feat", "fv_n", "valid", "nleft")}
    return RigBowSide(t["kps"], t["desc"], t["counts"], t["fv_node"], t["fv_ptr"], t["fv_feat"], t["fv_n"], 1, s["capacity"],
                      t["valid"] if with_valid else None, t["nleft"]), t


@pytest.mark.parametrize("path", ["default", "global trips"])
def test_recorded_rig_scenarios_through_the_device_form(tmp_path, monkeypatch, path):
    """bow_kf_frame_rig and bow_kf_kf_rig of tests/golden/matcher_world_ref.txt.gz, on the objects tests/support/rig_bow_dump.cpp rebuilds
    in this library's layout: the return values and every id of the vpMapPointMatches / vpMatches12 lines, through bow_pairs_device on a
    caller's stream.  On the global path the call is made a second time without b2a: the match row then lies in the handle's scratch."""
    import gzip
    import os
    from orb_slam3_modified_amd.rigbow import RigBowResult
    from tests import rigbow_world as rw
    from tests import world_util as wu
    gold = rw.recorded(gzip.open(os.path.join(wu.ROOT, "tests", "golden", "matcher_world_ref.txt.gz")).read().decode())
    rec = rw.dump(rw.golden_world(tmp_path), tmp_path)
    rb = _handle(monkeypatch, PATHS[path])
    s = torch.cuda.Stream(device=_dev())
    assert set(gold) == set(rw.SCENARIOS)
    for name in rw.SCENARIOS:
        b = rw.batch(rec, name)
        (sa, ka), (sb, kb) = _device_side(b["a"], True), _device_side(b["b"], b["mode"] == KEYFRAMES)
        tp = torch.from_numpy(b["pairs"]).to(_dev())
        torch.cuda.synchronize()
        out = rb.bow_pairs_device(sa, sb, tp, b["mode"], b["ratio"], b["ori"], stream=s.cuda_stream)
        s.synchronize()
        n, b2a, a2b = int(out.nmatches.cpu()[0]), out.b2a.cpu().numpy()[0], out.a2b.cpu().numpy()[0]
        assert n == gold[name][0] > 50, (name, n)
        assert np.array_equal(rw.ids_line(b, b2a, a2b), gold[name][1]), name
        wn, wb2a, wa2b = rw.model(b)
        assert n == wn and np.array_equal(b2a[:b["b"]["n"]], wb2a) and np.array_equal(a2b[:b["a"]["n"]], wa2b), name
        assert (b2a[b["b"]["n"]:] == -1).all() and (a2b[b["a"]["n"]:] == -1).all()
        if path != "default":
            only_a = RigBowResult(torch.zeros(1, dtype=torch.int32, device=_dev()), None, torch.zeros((1, b["a"]["capacity"], 2), dtype=torch.int32, device=_dev()))
            rb.bow_pairs_device(sa, sb, tp, b["mode"], b["ratio"], b["ori"], stream=s.cuda_stream, out=only_a)
            s.synchronize()
            assert int(only_a.nmatches.cpu()[0]) == n and np.array_equal(only_a.a2b.cpu().numpy()[0], a2b), name
    rb.close()


def fv_frames(fv, B):
    """The host FeatureVectors of a BowDeviceResult written without its BowVector group: [(None, {node: [features]})]."""
    fn, fp, ff, fc = (fv.fv_node.cpu().numpy().view(np.uint32), fv.fv_ptr.cpu().numpy(), fv.fv_feat.cpu().numpy().view(np.uint32),
                      fv.fv_n.cpu().numpy())
    return [(None, {int(fn[f, j]): ff[f, fp[f, j]:fp[f, j + 1]].astype(np.int64).tolist() for j in range(int(fc[f]))}) for f in range(B)]
