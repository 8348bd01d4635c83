"""The batched SearchForTriangulation (liborbx_trimatch.so, orb_slam3_modified_amd/trimatch.py) on the GPU: for every pair (nmatches,
matches12) equals tests/trimatch_model.py's, whole rows included -- on constructed inputs through the host form and on the buffers a batch
extraction and BowBatch.transform_device left in HBM (the batch of tests/trimatch_cases.py, whose inputs the CPU suite checks)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from orb_slam3_modified_amd import ORBextractor, ORBVocabulary, OrbxError, _lib
from orb_slam3_modified_amd._lib import KP_DTYPE
from orb_slam3_modified_amd.bow import BowBatch
from orb_slam3_modified_amd.trimatch import TriMatchBatch, TriMatchResult, TriMatchSide, lds_bytes, LDS_MAX
from tests import trimatch_cases as tc
from tests import trimatch_model as tm
from tests.test_trimatch_model import BOUNDARY_UNC, FREE, LINE_X0

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests.pair_batch_util import Batch as HbmBatch, dev  # noqa: E402


def _check_row(n, m12, want_n, want_m12, where):
    """One pair's row against the model's (nmatches, matches12 over the frame's features): the whole row."""
    k = len(want_m12)
    assert n == want_n, where
    assert np.array_equal(m12[:k], want_m12) and (m12[k:] == -1).all(), where
    assert n == (m12 >= 0).sum(), where


# ---- test 1: constructed inputs through the host form
CAP = 160
NODES = ({10: 1, 11: 5, 12: 64, 13: 65, 15: 25},       # frame 0: 160 features, as many as the capacity holds
         {10: 130, 11: 1, 12: 5, 13: 18, 16: 4},       # frame 1: 158 features; nodes 15 and 16 exist on one side only
         {})                                           # frame 2: empty


def _constructed():
    rng = np.random.default_rng(2024)
    base = {node: rng.integers(0, 256, 32).astype(np.uint8) for node in range(10, 17)}
    F = len(NODES)
    kps, desc = np.zeros((F, CAP), KP_DTYPE), np.zeros((F, CAP, 32), np.uint8)
    counts, fvs = np.zeros((F, 2), np.int32), []
    has, ur = (rng.random((F, CAP)) < 0.2).astype(np.uint8), np.full((F, CAP), -1.0, np.float32)
    for f, nodes in enumerate(NODES):
        n = sum(nodes.values())
        counts[f, 0] = n
        order = rng.permutation(n)                               # fv_feat is not in index order
        fv, at = {}, 0
        for node, size in nodes.items():
            fv[node] = [int(i) for i in order[at:at + size]]
            at += size
            for i in fv[node]:
                d = base[node].copy()
                for b in rng.integers(0, 256, int(rng.choice([0, 0, 8, 20, 30]))):   # no flipped bit at all: exact duplicates inside a node
                    d[b >> 3] ^= 1 << (b & 7)
                desc[f, i] = d
        fvs.append(fv)
        k = kps[f, :n]
        k["x"], k["y"] = rng.uniform(0, 320, n), rng.integers(0, 6, n) * 40.0 + rng.normal(0, 2.5, n)
        k["octave"], k["angle"] = rng.integers(0, 8, n), rng.choice([0.0, 0.0, 0.0, 30.0, 95.0, 200.0], n) + rng.normal(0, 2, n)
        near = rng.random(n) < 0.25                              # a cluster around (150, 81), where one geometry puts its epipole
        k["x"][near], k["y"][near] = 150.0 + rng.normal(0, 8, near.sum()), 81.0 + rng.normal(0, 2.5, near.sum())
        ur[f, :n] = np.where(rng.random(n) < 0.5, k["x"] - 4.0, -1.0)
    # the double comparison's boundary: frame 1's only feature of node 11 sits at x2 = 2 on octave 3, and a query of frame 0's node 11 has its
    # descriptor; with the line x = 0 as every query's epipolar line dsqr is 4 exactly
    ib, ia = fvs[1][11][0], fvs[0][11][2]
    kps[1, ib]["x"], kps[1, ib]["octave"] = 2.0, 3
    desc[1, ib] = desc[0, ia] = base[11]
    has[1, ib] = has[0, ia] = 0
    ur[1, ib] = ur[0, ia] = -1.0
    return kps, desc, counts, fvs, has, ur, (ia, ib)


def _pack(fvs, cap):
    """FeatureVector dicts as the four fixed-stride arrays."""
    F = len(fvs)
    node, ptr, feat, n = np.zeros((F, cap), np.uint32), np.zeros((F, cap + 1), np.int32), np.zeros((F, cap), np.uint32), np.zeros(F, np.int32)
    for f, fv in enumerate(fvs):
        at = 0
        for j, key in enumerate(sorted(fv)):
            node[f, j], ptr[f, j] = key, at
            feat[f, at:at + len(fv[key])] = fv[key]
            at += len(fv[key])
        n[f] = len(fv)
        ptr[f, len(fv):] = at
    return node, ptr, feat, n


def test_constructed_inputs_through_the_host_form():
    kps, desc, counts, fvs, has, ur, (qa, qb) = _constructed()
    node, ptr, feat, n = _pack(fvs, CAP)
    scale, sig = tc.level_tables()
    sig = sig.copy()
    sig[3] = BOUNDARY_UNC
    inside = tc.geometry_of("forward").copy()
    inside[9:11] = (150.0, 81.0)                                 # the epipole in a cluster of features
    naninf = FREE.copy()
    naninf[[2, 9, 10]] = (np.nan, np.inf, -np.inf)
    pairs9 = np.array([(0, 1), (1, 0), (0, 0), (1, 1), (0, 2), (2, 1), (2, 2), (1, 0), (0, 1)], np.int32)
    geom9 = np.stack([LINE_X0, tc.geometry_of("sideways"), tc.geometry_of("forward"), inside, FREE, FREE, FREE, inside, naninf])
    mb = TriMatchBatch(0)
    ties = matches = epipole = gate = 0
    for only_stereo, coarse, ori in itertools.product((False, True), repeat=3):
        for masks in ((has, ur), (None, None)) if not coarse else ((has, ur),):
            side = TriMatchSide(kps, desc, counts, node, ptr, feat, n, len(NODES), CAP, *masks)
            for pairs, geom in ((pairs9, geom9), (pairs9[:1], geom9[:1])):
                r = mb.pairs(side, side, pairs, geom, scale, sig, only_stereo, coarse, ori)
                for p, (ia, ib) in enumerate(pairs.tolist()):
                    na, nb = counts[ia, 0], counts[ib, 0]
                    st = {}
                    (ha, ua), (hb, ub) = ((None, None), (None, None)) if masks[0] is None else ((has[ia], ur[ia]), (has[ib], ur[ib]))
                    want = tm.search_for_triangulation(kps[ia, :na], desc[ia, :na], fvs[ia], ha, ua, kps[ib, :nb], desc[ib, :nb], fvs[ib], hb, ub,
                                                       geom[p], scale, sig, only_stereo, coarse, ori, stats=st)
                    _check_row(*r[p], *want, (only_stereo, coarse, ori, masks[0] is None, len(pairs), p))
                    ties += st["ties_last"]
                    matches += want[0]
                    epipole += st["epipole_rejected"]
                    gate += st["gate_rejected"]
                    if p == 0 and not only_stereo and not ori:   # the planted boundary: the double comparison lets it through
                        assert want[1][qa] == qb and r[p][1][qa] == qb
    assert ties > 0 and matches > 100 and epipole > 0 and gate > 0, (ties, matches, epipole, gate)
    # one float below the boundary the planted candidate fails: the model's comparison is the one under test
    sig[3] = np.nextafter(BOUNDARY_UNC, np.float32(0))
    side = TriMatchSide(kps, desc, counts, node, ptr, feat, n, len(NODES), CAP, has, ur)
    r = mb.pairs(side, side, pairs9[:1], geom9[:1], scale, sig, False, False, False)
    assert r[0][1][qa] != qb
    mb.close()


# ---- tests 2 - 5: extracted inputs on device buffers
class Batch(HbmBatch):
    """The extracted frames and, per levelsup, their FeatureVectors (device result + host dicts)."""

    def __init__(self, ex, imgs):
        super().__init__(ex, imgs)
        self.fv, self.hfv = {}, {}

    def transform(self, gv, levelsup):
        if levelsup not in self.fv:
            bb = BowBatch(gv, levelsup)
            self.fv[levelsup] = r = bb.transform_device(self.desc, self.counts, self.B, self.cap, stream=self.s.cuda_stream, bow=False)
            self.s.synchronize()
            bb.close()
            fn, fp, ff, fc = (r.fv_node.cpu().numpy().view(np.uint32), r.fv_ptr.cpu().numpy(), r.fv_feat.cpu().numpy().view(np.uint32),
                              r.fv_n.cpu().numpy())
            self.hfv[levelsup] = [{int(fn[f, j]): ff[f, fp[f, j]:fp[f, j + 1]].astype(np.int64).tolist() for j in range(int(fc[f]))}
                                  for f in range(self.B)]
        return self.fv[levelsup], self.hfv[levelsup]

    def side(self, fv, uright=None, **over):
        a = dict(kps=self.kps, desc=self.desc, counts=self.counts, fv_node=fv.fv_node, fv_ptr=fv.fv_ptr, fv_feat=fv.fv_feat, fv_n=fv.fv_n)
        a.update(over)
        return TriMatchSide(a["kps"], a["desc"], a["counts"], a["fv_node"], a["fv_ptr"], a["fv_feat"], a["fv_n"], self.B, self.cap, None, uright)


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """The batch, its vocabulary, the stereo mask and -- computed once -- the model's rows for (levelsup, stereo)."""
    ex = ORBextractor(*tc.EXTRACTOR, device_id=0)
    bt = Batch(ex, tc.frames())
    assert (bt.hc[:, 0] > 250).all() and lds_bytes(bt.cap, bt.cap) <= LDS_MAX
    gv = ORBVocabulary(ex)
    assert gv.loadFromTextFile(tc.vocabulary_file(str(tmp_path_factory.mktemp("voc") / "voc.txt"), [bt.frame(f)[1] for f in range(bt.B)]))
    hur = np.stack([tc.stereo_uright(bt.hk[f]["x"], f) for f in range(bt.B)])
    tur = torch.from_numpy(hur).to(dev())
    scale, sig = tc.level_tables()
    pairs, geom = tc.pairs(), tc.geom_rows()
    want = {}
    for levelsup in tc.LEVELSUP:
        _, hfv = bt.transform(gv, levelsup)
        if levelsup == tc.VOC_L:
            assert all(list(d) == [0] for d in hfv)              # one node: every feature against every feature
        for stereo in (False, True):
            rows = []
            for p, (ia, ib) in enumerate(pairs.tolist()):
                (ka, da), (kb, db) = bt.frame(ia), bt.frame(ib)
                rows.append(tm.search_for_triangulation(ka, da, hfv[ia], None, hur[ia] if stereo else None, kb, db, hfv[ib], None,
                                                        hur[ib] if stereo else None, geom[p], scale, sig, False, False, True))
            assert sum(n for n, _ in rows) > 500
            want[levelsup, stereo] = rows
    return dict(bt=bt, gv=gv, tur=tur, hur=hur, scale=scale, sig=sig, pairs=pairs, geom=geom, want=want,
                tp=torch.from_numpy(pairs).to(dev()), tg=torch.from_numpy(geom).to(dev()))


def _run(mb, s, a, b, tp, tg, stream, only_stereo=False, coarse=False, ori=True):
    out = mb.pairs_device(a, b, tp, tg, s["scale"], s["sig"], only_stereo, coarse, ori, stream=stream.cuda_stream)
    stream.synchronize()
    return out.nmatches.cpu().numpy(), out.matches12.cpu().numpy()


def _all_cases(s, mb):
    bt = s["bt"]
    for levelsup in tc.LEVELSUP:
        fv, _ = bt.transform(s["gv"], levelsup)
        for stereo in (False, True):
            side = bt.side(fv, s["tur"] if stereo else None)
            yield (levelsup, stereo), _run(mb, s, side, side, s["tp"], s["tg"], bt.s)


def test_extracted_inputs_on_device_buffers(small):
    mb = TriMatchBatch(0)
    for key, (n, m12) in _all_cases(small, mb):
        for p, (wn, wm12) in enumerate(small["want"][key]):
            _check_row(n[p], m12[p], wn, wm12, key + (p,))
    mb.close()


def test_the_global_path_gives_the_same_rows(small, monkeypatch):
    monkeypatch.setenv("ORBX_TRIMATCH_LDS", "0")
    glob = TriMatchBatch(0)
    monkeypatch.delenv("ORBX_TRIMATCH_LDS")
    lds = TriMatchBatch(0)
    for (key, (n, m12)), (_, (gn, gm12)) in zip(_all_cases(small, lds), _all_cases(small, glob)):
        assert (n > 0).all() and n.tobytes() == gn.tobytes() and m12.tobytes() == gm12.tobytes(), key
        for p, (wn, wm12) in enumerate(small["want"][key]):
            _check_row(gn[p], gm12[p], wn, wm12, ("global",) + key + (p,))
    glob.close()
    lds.close()


def test_malformed_pairs(small):
    s, bt = small, small["bt"]
    fv, hfv = bt.transform(s["gv"], 1)
    mb = TriMatchBatch(0)
    F = bt.B
    counts, fv_feat, kps = bt.counts.clone(), fv.fv_feat.clone(), bt.kps.clone()
    counts[3, 0] = bt.cap + 1                                    # a count above the capacity
    fv_feat[8, 17] = int(bt.hc[8, 0])                            # an entry that is not below its frame's count
    listed = hfv[5][sorted(hfv[5])[2]][0]
    kps[5, listed, 20:24] = torch.tensor([8, 0, 0, 0], dtype=torch.uint8, device=dev())   # an octave that is no level
    assert KP_DTYPE.fields["octave"][1] == 20
    bad_side = bt.side(fv, None, counts=counts, fv_feat=fv_feat, kps=kps)
    good = bt.side(fv)
    pairs = np.array([(0, 1), (0, F), (1, 2), (-1, 1), (2, 3), (3, 4), (4, 6), (4, 5), (5, 6), (6, 7), (7, 8), (8, 9), (9, 10), (F + 100, 0), (10, 11)],
                     np.int32)
    # (4, 5): frame 5 is side B, its listed feature's octave is read; (5, 6): frame 5 as side A reads no octave
    bad = {1, 3, 4, 5, 7, 10, 11, 13}
    tg = torch.from_numpy(np.stack([tc.geometry_of("sideways")] * len(pairs))).to(dev())
    n, m12 = _run(mb, s, bad_side, bad_side, torch.from_numpy(pairs).to(dev()), tg, bt.s)
    wn, wm12 = _run(mb, s, good, good, torch.from_numpy(np.clip(pairs, 0, F - 1)).to(dev()), tg, bt.s)
    for i in range(len(pairs)):
        if i in bad:
            assert n[i] == -1 and (m12[i] == -1).all(), i
        else:                                                    # the neighbours are what they are without the malformed pairs
            assert n[i] == wn[i] > 0 and np.array_equal(m12[i], wm12[i]), i
    # what the host can check: ORBX_E_INVALID with a reason
    M = _lib.trimatch_lib()
    sa = good._struct()
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    fp = C.POINTER(C.c_float)
    out = TriMatchResult(torch.zeros(len(pairs), dtype=torch.int32, device=dev()), torch.zeros((len(pairs), bt.cap), dtype=torch.int32, device=dev()))
    ok = [C.byref(sa), C.byref(sa), p(s["tp"]), 2, p(tg), s["scale"].ctypes.data_as(fp), s["sig"].ctypes.data_as(fp), 8, 0, 0, 1, p(out.matches12),
          p(out.nmatches), None]
    assert M.orbx_trimatch_pairs_device(mb._h, *ok) == 0
    for idx, v in ((0, None), (2, None), (3, 0), (4, None), (5, None), (6, None), (7, 0), (7, 17), (11, None), (12, None)):
        a_ = list(ok)
        a_[idx] = v
        assert M.orbx_trimatch_pairs_device(mb._h, *a_) == _lib.ORBX_E_INVALID, (idx, v)
        assert len(M.orbx_trimatch_last_error(mb._h)) > 10
    for field, v in (("d_desc", None), ("d_fv_n", None), ("nframes", 0), ("capacity", 0), ("capacity", 65537), ("d_kps", None)):
        sb = good._struct()
        setattr(sb, field, v)
        a_ = list(ok)
        a_[1] = C.byref(sb)
        assert M.orbx_trimatch_pairs_device(mb._h, *a_) == _lib.ORBX_E_INVALID, field
    with pytest.raises(OrbxError):
        mb.pairs_device(good, good, s["tp"], s["tg"], s["scale"][:0], s["sig"][:0])
    bt.s.synchronize()
    mb.close()
    mb.close()


def test_the_device_form_on_a_callers_stream_equals_the_host_form(small):
    s, bt = small, small["bt"]
    fv, _ = bt.transform(s["gv"], 1)
    mb = TriMatchBatch(0)
    host = lambda t: t.cpu().numpy()   # noqa: E731
    hs = TriMatchSide(bt.hk, bt.hd, bt.hc, host(fv.fv_node), host(fv.fv_ptr), host(fv.fv_feat), host(fv.fv_n), bt.B, bt.cap, None, s["hur"])
    mine = torch.cuda.Stream(device=dev())
    torch.cuda.synchronize()
    for only_stereo, coarse, ori in ((False, False, True), (True, False, False), (False, True, True)):
        r = mb.pairs(hs, hs, s["pairs"], s["geom"], s["scale"], s["sig"], only_stereo, coarse, ori)
        side = bt.side(fv, s["tur"])
        n, m12 = _run(mb, s, side, side, s["tp"], s["tg"], mine, only_stereo, coarse, ori)
        assert np.array_equal(r.nmatches, n) and np.array_equal(r.matches12, m12) and (n > 0).all()
        k, row = r[2]
        assert k == n[2] and np.array_equal(row, m12[2]) and len(r.matched_pairs(2)) == k
    mb.close()
