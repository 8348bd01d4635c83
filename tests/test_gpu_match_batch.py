"""The batched SearchByBoW (liborbx_match.so, orb_slam3_modified_amd/match.py) on the GPU: for every pair the matches equal the oracle's
ORBmatcher::SearchByBoW and the per-pair orbx_search_by_bow (frame mode) resp. tests/match_batch_model.py (keyframe mode), on the buffers a
batch extraction and BowBatch.transform_device left in HBM, and on the constructed batch of tests/match_batch_cases.py (hand-written
FeatureVectors, every planted node on every path)."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as po
from orb_slam3_modified_amd import ORBextractor, ORBmatcher, ORBVocabulary, OrbxError, _lib, synth
from orb_slam3_modified_amd.bow import BowBatch
from orb_slam3_modified_amd.match import FRAME, KEYFRAMES, MatchBatch, MatchSide
from tests import match_batch_model as mm
from tests.vocab_util import make_vocabulary

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests.pair_batch_util import EUROC, VGA5K, Batch as HbmBatch, dev, pairs256  # noqa: E402


class Batch(HbmBatch):
    """The extracted frames and, per levelsup, their FeatureVectors (device result + host dicts)."""

    def __init__(self, ex, imgs):
        super().__init__(ex, imgs)
        self.fv, self.hfv = {}, {}

    def transform(self, gv, key, levelsup):
        if key not in self.fv:
            bb = BowBatch(gv, levelsup)
            self.fv[key] = bb.transform_device(self.desc, self.counts, self.B, self.cap, stream=self.s.cuda_stream, bow=False)
            self.s.synchronize()
            bb.close()
            r = self.fv[key]
            fn, fp, ff, fc = (r.fv_node.cpu().numpy().view(np.uint32), r.fv_ptr.cpu().numpy(), r.fv_feat.cpu().numpy().view(np.uint32),
                              r.fv_n.cpu().numpy())
            self.hfv[key] = [{int(fn[f, j]): ff[f, fp[f, j]:fp[f, j + 1]].astype(np.int64).tolist() for j in range(int(fc[f]))}
                             for f in range(self.B)]
        return self.fv[key], self.hfv[key]

    def side(self, fv, valid=None, lo=0, hi=None):
        hi = self.B if hi is None else hi
        return MatchSide(self.kps[lo:hi], self.desc[lo:hi], self.counts[lo:hi], fv.fv_node[lo:hi], fv.fv_ptr[lo:hi], fv.fv_feat[lo:hi], fv.fv_n[lo:hi],
                         hi - lo, self.cap, None if valid is None else valid[lo:hi])


def _voc(ex, tmp_path_factory, train, k, L, seed):
    p = str(tmp_path_factory.mktemp("voc") / f"voc_{k}_{L}.txt")
    make_vocabulary(p, train, k, L, seed=seed)
    gv = ORBVocabulary(ex)
    assert gv.loadFromTextFile(p)
    return gv


@pytest.fixture(scope="module")
def euroc(tmp_path_factory):
    ex = ORBextractor(*EUROC[2], device_id=0)
    bt = Batch(ex, synth.make_stream(256, EUROC[0], EUROC[1]))
    assert (bt.hc[:, 0] > 800).all()
    train = np.concatenate([bt.hd[f, :bt.hc[f, 0]] for f in range(4)])
    vocs = {(10, 4): _voc(ex, tmp_path_factory, train, 10, 4, 104), (10, 6): _voc(ex, tmp_path_factory, train, 10, 6, 106)}
    return bt, vocs


def _mask(bt, seed, frac=0.7):
    rng = np.random.default_rng(seed)
    hv = (rng.random((bt.B, bt.cap)) < frac).astype(np.uint8)
    return torch.from_numpy(hv).to(dev()), hv


def _run(mb, a, b, pairs, mode, ratio, ori, stream):
    tp = torch.from_numpy(np.ascontiguousarray(pairs, np.int32)).to(dev())
    out = mb.bow_pairs_device(a, b, tp, mode, ratio, ori, stream=stream.cuda_stream)
    stream.synchronize()
    return out.nmatches.cpu().numpy(), out.b2a.cpu().numpy(), out.a2b.cpu().numpy()


def _check_rows(n, b2a, a2b, want_n, want_b2a, na, where):
    """One pair's rows against the expected (nmatches, b2a over the frame's features): whole rows, and a2b the exact inverse."""
    nb = len(want_b2a)
    assert n == want_n, where
    assert np.array_equal(b2a[:nb], want_b2a) and (b2a[nb:] == -1).all(), where
    assert np.array_equal(a2b[:na], mm.invert(want_b2a, na)) and (a2b[na:] == -1).all(), where
    assert n == (b2a >= 0).sum() == (a2b >= 0).sum(), where


def _oracle(bta, hfa, ia, hva, btb, hfb, ib, ratio, ori):
    (ka, da), (kb, db) = bta.frame(ia), btb.frame(ib)
    aa, ab = ka["angle"], kb["angle"]
    valid = np.ones(len(da), np.uint8) if hva is None else hva[ia, :len(da)]
    return po.search_by_bow(da, aa, valid, hfa[ia], db, ab, hfb[ib], ratio, ori), (da, aa, valid, db, ab)


# ratio 0.6 / 0.7 / 0.9, orientation on and off, valid_a NULL and a 70 % mask: every value with every levelsup through the rotation below
COMBOS = [(0.7, True, False), (0.6, True, True), (0.9, False, True), (0.7, False, False), (0.9, True, False), (0.6, False, True)]


@pytest.mark.parametrize("k,L", [(10, 4), (10, 6)])
def test_parity_per_pair_frame_mode(euroc, k, L):
    bt, vocs = euroc
    gv = vocs[k, L]
    mb = MatchBatch(0)
    tv, hv = _mask(bt, 11)
    p256 = pairs256()
    step = 0
    for levelsup in sorted({0, 2, 4, L}):
        fv, hfv = bt.transform(gv, (k, L, levelsup), levelsup)
        if levelsup == L:
            assert all(list(d) == [0] for d in hfv[:8])                 # one node: every feature against every feature
        for P, split in ((256, False), (7, True), (1, False), (7, False)):
            ratio, ori, masked = COMBOS[step % len(COMBOS)]
            step += 1
            vac = P == 256 and (k, L, levelsup) == (10, 6, 4)           # the case whose inputs are checked below
            if P == 256:
                ratio, ori, masked = (0.7, True, False) if vac else (ratio, ori, masked)
                pairs = p256
            else:
                pairs = np.array([(0, 1), (10, 15), (20, 20), (7, 9), (7, 30), (100, 101), (250, 255)][:P], np.int32)
            valid, hvalid = (tv, hv) if masked else (None, None)
            if split:        # A and B as two batches: B is the upper half of the frames
                a, b, off = bt.side(fv, valid, 0, 128), bt.side(fv, None, 128, 256), 128
                pairs = np.array([(0, 1), (10, 15), (20, 20), (7, 9), (7, 30), (100, 101), (120, 127)], np.int32)
            else:
                a, b, off = bt.side(fv, valid), bt.side(fv), 0
            n, b2a, a2b = _run(mb, a, b, pairs, FRAME, ratio, ori, bt.s)
            where = (k, L, levelsup, P, split, ratio, ori, masked)
            m = ORBmatcher(bt.ex, ratio, ori)
            got_ge20 = removed = contended = 0
            for i, (ia, ib) in enumerate(pairs.tolist()):
                ib += off
                (on, ob2a), (da, aa, va, db, ab) = _oracle(bt, hfv, ia, hvalid, bt, hfv, ib, ratio, ori)
                _check_rows(n[i], b2a[i], a2b[i], on, ob2a, len(da), where + (i,))
                if P != 256 or i % 23 == 0:    # the per-pair entry point of before, on the pair's host copies
                    sn, sb2a = m.SearchByBoW(da, aa, va, hfv[ia], db, ab, hfv[ib])
                    assert sn == on and np.array_equal(sb2a, ob2a), where + (i, "orbx_search_by_bow")
                if vac and i < 200:
                    got_ge20 += on >= 20
                    on_off, _ = po.search_by_bow(da, aa, va, hfv[ia], db, ab, hfv[ib], ratio, False)
                    removed += on_off > on
                    if i % 10 == 0:
                        st = {}
                        mm.search_by_bow(da, aa, va, hfv[ia], db, ab, None, hfv[ib], FRAME, ratio, ori, stats=st)
                        contended += st["contended"]
            if vac:
                # the inputs exercise what the test is about, on the ORACLE's results
                assert got_ge20 >= 180, got_ge20
                assert removed >= 1 and contended >= 1, (removed, contended)
    mb.close()


def test_another_capacity_and_the_existing_search_by_bow_setup(tmp_path_factory):
    """640 x 480 at 5000 features (mpIniORBextractor): the setup of test_search_by_bow_equals_oracle; this capacity does not fit the LDS."""
    ex = ORBextractor(*VGA5K[2], device_id=0)
    bt = Batch(ex, synth.make_stream(3))
    assert bt.cap != ORBextractor(*EUROC[2], device_id=0).capacity and (bt.hc[:, 0] > 3000).all()
    gv = _voc(ex, tmp_path_factory, np.concatenate([bt.hd[f, :bt.hc[f, 0]] for f in range(3)]), 10, 4, 5)
    mb = MatchBatch(0)
    tv, hv = _mask(bt, 72)
    for levelsup, pairs in ((2, [(0, 1), (2, 1)]), (0, [(0, 1), (2, 1), (1, 1)]), (4, [(0, 1)])):
        fv, hfv = bt.transform(gv, levelsup, levelsup)
        for ratio, ori, masked in ((0.7, True, True), (0.9, False, False)):
            valid, hvalid = (tv, hv) if masked else (None, None)
            n, b2a, a2b = _run(mb, bt.side(fv, valid), bt.side(fv), np.array(pairs, np.int32), FRAME, ratio, ori, bt.s)
            m = ORBmatcher(ex, ratio, ori)
            total = 0
            for i, (ia, ib) in enumerate(pairs):
                (on, ob2a), (da, aa, va, db, ab) = _oracle(bt, hfv, ia, hvalid, bt, hfv, ib, ratio, ori)
                _check_rows(n[i], b2a[i], a2b[i], on, ob2a, len(da), (levelsup, ratio, ori, i))
                sn, sb2a = m.SearchByBoW(da, aa, va, hfv[ia], db, ab, hfv[ib])
                assert sn == on and np.array_equal(sb2a, ob2a)
                total += on
            if levelsup == 2 and ratio == 0.7:
                assert total > 100, total      # the oracle's matches over the two pairs of the existing test's setup
    mb.close()


def test_keyframe_mode_equals_the_model(euroc):
    bt, vocs = euroc
    gv = vocs[10, 4]
    mb = MatchBatch(0)
    tva, hva = _mask(bt, 21)
    tvb, hvb = _mask(bt, 22, 0.6)
    pairs = np.array([(0, 1), (3, 8), (5, 5), (40, 41), (7, 12), (200, 201)], np.int32)
    differ = 0
    for levelsup, ratio, ori in ((2, 0.7, True), (0, 0.9, False), (4, 0.6, True)):
        fv, hfv = bt.transform(gv, (10, 4, levelsup), levelsup)
        for va, vb in (((tva, hva), (tvb, hvb)), ((None, None), (tvb, hvb)), ((tva, hva), (None, None))):
            n, b2a, a2b = _run(mb, bt.side(fv, va[0]), bt.side(fv, vb[0]), pairs, KEYFRAMES, ratio, ori, bt.s)
            nf, b2af, _ = _run(mb, bt.side(fv, va[0]), bt.side(fv, vb[0]), pairs, FRAME, ratio, ori, bt.s)
            for i, (ia, ib) in enumerate(pairs.tolist()):
                (ka, da), (kb, db) = bt.frame(ia), bt.frame(ib)
                aa, ab = ka["angle"], kb["angle"]
                hva_i = None if va[1] is None else va[1][ia, :len(da)]
                hvb_i = None if vb[1] is None else vb[1][ib, :len(db)]
                wn, wb2a = mm.search_by_bow(da, aa, hva_i, hfv[ia], db, ab, hvb_i, hfv[ib], KEYFRAMES, ratio, ori)
                _check_rows(n[i], b2a[i], a2b[i], wn, wb2a, len(da), ("keyframes", levelsup, ratio, ori, i))
                if hvb_i is not None:
                    assert hvb_i[np.nonzero(wb2a >= 0)[0]].all()
                fn, fb2a = mm.search_by_bow(da, aa, hva_i, hfv[ia], db, ab, hvb_i, hfv[ib], FRAME, ratio, ori)
                _check_rows(nf[i], b2af[i], mm.invert(b2af[i], bt.cap), fn, fb2a, len(da), ("frame, valid_b ignored", levelsup, i))
                differ += not np.array_equal(fb2a, wb2a)
    assert differ >= 1       # the model's two modes disagree on some pair: the mode reaches the kernel
    mb.close()


def test_both_paths_give_the_same_bytes(euroc, monkeypatch):
    bt, vocs = euroc
    gv = vocs[10, 6]
    tv, _ = _mask(bt, 31)
    pairs = pairs256()[::8]
    default = MatchBatch(0)
    handles = {}
    for name, env in (("global", {"ORBX_MATCH_LDS": "0"}), ("trips", {"ORBX_MATCH_WAVE_NODE": "3"}), ("global trips", {"ORBX_MATCH_LDS": "0", "ORBX_MATCH_WAVE_NODE": "0"})):
        for k_, v_ in env.items():
            monkeypatch.setenv(k_, v_)
        handles[name] = MatchBatch(0)
        for k_ in env:
            monkeypatch.delenv(k_)
    for levelsup, mode in ((4, FRAME), (2, KEYFRAMES), (6, FRAME), (0, KEYFRAMES)):
        fv, _ = bt.transform(gv, (10, 6, levelsup), levelsup)
        a, b = bt.side(fv, tv), bt.side(fv, tv)
        ref = _run(default, a, b, pairs, mode, 0.7, True, bt.s)
        assert (ref[0] > 0).any()
        for name, h in handles.items():
            got = _run(h, a, b, pairs, mode, 0.7, True, bt.s)
            for x, y in zip(ref, got):
                assert x.tobytes() == y.tobytes(), (name, levelsup, mode)
    for h in list(handles.values()) + [default]:
        h.close()


def test_malformed_pairs(euroc):
    bt, vocs = euroc
    fv, hfv = bt.transform(vocs[10, 4], (10, 4, 2), 2)
    mb = MatchBatch(0)
    F = 12
    counts, fv_n, fv_feat = bt.counts[:F].clone(), fv.fv_n[:F].clone(), fv.fv_feat[:F].clone()
    counts[3, 0] = -1                                     # an overflowed frame
    fv_n[5] = -1                                          # a frame without a FeatureVector
    fv_feat[8, 17] = int(bt.hc[8, 0])                     # an entry that is not below its frame's count
    side = MatchSide(bt.kps[:F], bt.desc[:F], counts, fv.fv_node[:F], fv.fv_ptr[:F], fv_feat, fv_n, F, bt.cap)
    good = MatchSide(bt.kps[:F], bt.desc[:F], bt.counts[:F], fv.fv_node[:F], fv.fv_ptr[:F], fv.fv_feat[:F], fv.fv_n[:F], F, bt.cap)
    pairs = np.array([(0, 1), (0, F), (1, 2), (-1, 1), (2, 3), (3, 4), (4, 6), (5, 6), (6, 5), (6, 7), (7, 8), (8, 9), (9, 10), (F + 100, 0), (10, 11)], np.int32)
    bad = {1, 3, 4, 5, 7, 8, 10, 11, 13}
    n, b2a, a2b = _run(mb, side, side, pairs, FRAME, 0.7, True, bt.s)
    wn, wb2a, wa2b = _run(mb, good, good, np.clip(pairs, 0, F - 1), FRAME, 0.7, True, bt.s)
    for i in range(len(pairs)):
        if i in bad:
            assert n[i] == -1 and (b2a[i] == -1).all() and (a2b[i] == -1).all(), i
        else:                                             # the neighbours are what they are without the malformed pairs
            assert n[i] == wn[i] > 0 and np.array_equal(b2a[i], wb2a[i]) and np.array_equal(a2b[i], wa2b[i]), i
    # either output alone
    tp = torch.from_numpy(pairs).to(dev())
    from orb_slam3_modified_amd.match import MatchResult
    only_b = MatchResult(torch.zeros(len(pairs), dtype=torch.int32, device=dev()), torch.zeros((len(pairs), bt.cap), dtype=torch.int32, device=dev()), None)
    only_a = MatchResult(torch.zeros(len(pairs), dtype=torch.int32, device=dev()), None, torch.zeros((len(pairs), bt.cap), dtype=torch.int32, device=dev()))
    mb.bow_pairs_device(side, side, tp, FRAME, 0.7, True, stream=bt.s.cuda_stream, out=only_b)
    mb.bow_pairs_device(side, side, tp, FRAME, 0.7, True, stream=bt.s.cuda_stream, out=only_a)
    bt.s.synchronize()
    assert np.array_equal(only_b.b2a.cpu().numpy(), b2a) and np.array_equal(only_a.a2b.cpu().numpy(), a2b)
    assert np.array_equal(only_b.nmatches.cpu().numpy(), n) and np.array_equal(only_a.nmatches.cpu().numpy(), n)
    # what the host can check: ORBX_E_INVALID with a reason
    M = _lib.match_lib()
    sa = good._struct()
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    o = only_b
    ok = [C.byref(sa), C.byref(sa), p(tp), len(pairs), FRAME, 0.7, 1, p(o.b2a), None, p(o.nmatches), None]
    assert M.orbx_match_bow_pairs_device(mb._h, *ok) == 0
    for idx, v in ((0, None), (2, None), (3, 0), (3, -2), (4, 2), (4, -1), (7, None), (9, None)):
        a_ = list(ok)
        a_[idx] = v
        assert M.orbx_match_bow_pairs_device(mb._h, *a_) == _lib.ORBX_E_INVALID, (idx, v)
        assert len(M.orbx_match_last_error(mb._h)) > 10
    for field, v in (("d_desc", None), ("d_fv_n", None), ("nframes", 0), ("capacity", 0), ("d_kps", None)):
        sb = good._struct()
        setattr(sb, field, v)
        a_ = list(ok)
        a_[1] = C.byref(sb)
        assert M.orbx_match_bow_pairs_device(mb._h, *a_) == _lib.ORBX_E_INVALID, field
    with pytest.raises(OrbxError):
        mb.bow_pairs_device(good, good, tp, 5, 0.7, True)
    bt.s.synchronize()
    mb.close()
    mb.close()


def test_host_form_equals_device_form(euroc):
    bt, vocs = euroc
    fv, hfv = bt.transform(vocs[10, 4], (10, 4, 2), 2)
    mb = MatchBatch(0)
    F = 9
    tv, hv = _mask(bt, 41)
    pairs = np.array([(0, 1), (1, 0), (4, 4), (2, 8), (8, 3)], np.int32)
    host = lambda t: t[:F].cpu().numpy()   # noqa: E731
    ha = MatchSide(bt.hk[:F], bt.hd[:F], bt.hc[:F], host(fv.fv_node), host(fv.fv_ptr), host(fv.fv_feat), host(fv.fv_n), F, bt.cap, hv[:F])
    hb = MatchSide(bt.hk[:F], bt.hd[:F], bt.hc[:F], host(fv.fv_node), host(fv.fv_ptr), host(fv.fv_feat), host(fv.fv_n), F, bt.cap, None)
    for mode, (sa, sb) in ((FRAME, (ha, hb)), (KEYFRAMES, (hb, ha)), (FRAME, (hb, hb))):
        r = mb.bow_pairs(sa, sb, pairs, mode, 0.7, True)
        da = bt.side(fv, None if sa.valid is None else tv, 0, F)
        db = bt.side(fv, None if sb.valid is None else tv, 0, F)
        n, b2a, a2b = _run(mb, da, db, pairs, mode, 0.7, True, bt.s)
        assert np.array_equal(r.nmatches, n) and np.array_equal(r.b2a, b2a) and np.array_equal(r.a2b, a2b) and (n > 0).all()
        k, rb, ra = r[2]
        assert k == n[2] and np.array_equal(rb, b2a[2]) and np.array_equal(ra, a2b[2])
    mb.close()


def test_two_calls_back_to_back_on_two_streams(euroc, monkeypatch):
    """Calls on one handle share its scratch: the second waits for the first, whatever streams they are on."""
    bt, vocs = euroc
    fv2, _ = bt.transform(vocs[10, 6], (10, 6, 2), 2)
    fv6, _ = bt.transform(vocs[10, 6], (10, 6, 6), 6)
    p1, p2 = pairs256(), pairs256()[::-1].copy()
    alone = MatchBatch(0)
    w1 = _run(alone, bt.side(fv6), bt.side(fv6), p1, FRAME, 0.7, True, bt.s)
    w2 = _run(alone, bt.side(fv2), bt.side(fv2), p2, KEYFRAMES, 0.9, False, bt.s)
    alone.close()
    monkeypatch.setenv("ORBX_MATCH_LDS", "0")             # the global-memory path: both calls use the handle's scratch
    mb = MatchBatch(0)
    monkeypatch.delenv("ORBX_MATCH_LDS")
    s1, s2 = torch.cuda.Stream(device=dev()), torch.cuda.Stream(device=dev())
    t1, t2 = torch.from_numpy(p1).to(dev()), torch.from_numpy(p2).to(dev())
    torch.cuda.synchronize()
    r1 = mb.bow_pairs_device(bt.side(fv6), bt.side(fv6), t1, FRAME, 0.7, True, stream=s1.cuda_stream)
    r2 = mb.bow_pairs_device(bt.side(fv2), bt.side(fv2), t2, KEYFRAMES, 0.9, False, stream=s2.cuda_stream)
    s1.synchronize()
    s2.synchronize()
    for r, w in ((r1, w1), (r2, w2)):
        assert np.array_equal(r.nmatches.cpu().numpy(), w[0]) and np.array_equal(r.b2a.cpu().numpy(), w[1]) and np.array_equal(r.a2b.cpu().numpy(), w[2])
    mb.close()


# ---- the constructed batch of tests/match_batch_cases.py: every planted node through the kernel, whole rows, on every path
from tests import match_batch_cases as mc  # noqa: E402

MC_COMBOS = [(mode, valid, ori) for mode in (FRAME, KEYFRAMES) for valid in (True, False) for ori in (True, False)]
MC_PATHS = {"default": {}, "global": {"ORBX_MATCH_LDS": "0"}, "trips": {"ORBX_MATCH_WAVE_NODE": "3"},
            "global trips": {"ORBX_MATCH_LDS": "0", "ORBX_MATCH_WAVE_NODE": "0"}}


@pytest.fixture(scope="module")
def constructed():
    """The batch and -- computed once -- the model's whole rows (nmatches, b2a, a2b) under every run, mode, valid form and
    check_orientation.  A malformed pair: -1 and rows of -1."""
    c = mc.build()
    P = len(mc.PAIRS)
    for run, ratio in mc.RUNS.items():
        for mode, valid, ori in MC_COMBOS:
            n, b2a, a2b = np.full(P, -1, np.int32), np.full((P, mc.CAP), -1, np.int32), np.full((P, mc.CAP), -1, np.int32)
            for p, (ia, ib) in enumerate(mc.PAIRS.tolist()):
                if p in mc.MALFORMED:
                    continue
                (da, aa, va, fa), (db, ab, vb, fb) = mc.frame(c, ia), mc.frame(c, ib)
                n[p], row = mm.search_by_bow(da, aa, va if valid else None, fa, db, ab, vb if valid else None, fb, mode, ratio, ori)
                b2a[p, :len(db)], a2b[p, :len(da)] = row, mm.invert(row, len(da))
            c["want", run, mode, valid, ori] = (n, b2a, a2b)
    return c


@pytest.mark.parametrize("path", list(MC_PATHS))
def test_constructed_batch_through_the_host_form(constructed, monkeypatch, path):
    """Both modes, both forms of `valid`, with and without check_orientation, every nn_ratio of the batch, through MatchBatch.bow_pairs.
    "trips" and "global trips" put the 63- and 64-candidate nodes (and every smaller one) through the trip loop."""
    c = constructed
    for k_, v_ in MC_PATHS[path].items():
        monkeypatch.setenv(k_, v_)
    mb = MatchBatch(0)
    for k_ in MC_PATHS[path]:
        monkeypatch.delenv(k_)
    for run, ratio in mc.RUNS.items():
        for mode, valid, ori in MC_COMBOS:
            side = MatchSide(c["kps"], c["desc"], c["counts"], c["fv_node"], c["fv_ptr"], c["fv_feat"], c["fv_n"], mc.K, mc.CAP, c["valid"] if valid else None)
            r = mb.bow_pairs(side, side, mc.PAIRS, mode, ratio, ori)
            for g, w, name in zip((r.nmatches, r.b2a, r.a2b), c["want", run, mode, valid, ori], ("nmatches", "b2a", "a2b")):
                bad = np.nonzero((g != w).reshape(len(w), -1).any(1))[0]
                assert len(bad) == 0, (path, run, mode, valid, ori, name, bad.tolist())
            for name, (p, crun, want) in mc.CLAIMS.items():           # the named outcomes, read off the kernel's rows
                if crun == run and (ori or p not in (mc.P_ROT1, mc.P_ROT2)):
                    w = want(mode, valid)
                    assert r.a2b[p, mc.PLANTED[name]] == (-1 if w is None else mc.KP[w]), (path, name, mode, valid, ori)
            for p in mc.MALFORMED:
                assert r.nmatches[p] == -1 and (r.b2a[p] == -1).all() and (r.a2b[p] == -1).all(), p
    mb.close()


def test_constructed_pairs_through_the_per_pair_entry_point(constructed):
    """Frame mode: every well-formed pair equals orbx_search_by_bow (ORBmatcher.SearchByBoW) of the pair, which takes the hand-built
    FeatureVectors as they are.  The two pairs with an empty FeatureVector on one side are left to the model: that entry point is not
    given zero-length arrays here."""
    c = constructed
    ex = ORBextractor(*EUROC[2], device_id=0)
    done = 0
    for run, ratio in mc.RUNS.items():
        for valid in (True, False):
            for ori in (True, False):
                m = ORBmatcher(ex, ratio, ori)
                n, b2a, _ = c["want", run, FRAME, valid, ori]
                for p, (ia, ib) in enumerate(mc.PAIRS.tolist()):
                    if p in mc.MALFORMED or p in (mc.P_NOFV_A, mc.P_NOFV_B):
                        continue
                    (da, aa, va, fa), (db, ab, _, fb) = mc.frame(c, ia), mc.frame(c, ib)
                    sn, sb2a = m.SearchByBoW(da, aa, va if valid else np.ones(len(da), np.uint8), fa, db, ab, fb)
                    assert sn == n[p] and np.array_equal(sb2a, b2a[p, :len(db)]), (run, valid, ori, p)
                    done += 1
    assert done == len(mc.RUNS) * 4 * (len(mc.PAIRS) - len(mc.MALFORMED) - 2)
