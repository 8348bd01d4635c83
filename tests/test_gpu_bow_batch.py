"""The batched bag of words (liborbx_bow.so, orb_slam3_modified_amd/bow.py) on the GPU: per frame the BowVector and the FeatureVector equal the
oracle's TemplatedVocabulary::transform and the single-frame path (orbx_bow_transform + orbx_bow_finalize) byte for byte, on the buffers a
batch extraction or a replay step left in HBM; the score matrix equals orbx_bow_score_l1 entry by entry as raw bits."""
import ctypes as C
import gc

import numpy as np
import pytest

from oracle import pyoracle as po
from orb_slam3_modified_amd import ORBextractor, ORBVocabulary, OrbxError, _lib, synth
from orb_slam3_modified_amd.bow import BowBatch
from orb_slam3_modified_amd.vocabulary import BINARY, DOT_PRODUCT, IDF, L2_NORM, TF, TF_IDF
from tests.vocab_util import make_vocabulary

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EUROC = (480, 752, (1000, 1.2, 8, 20, 7))
VGA15 = (480, 640, (1500, 1.2, 8, 20, 7))


def _dev():
    return torch.device("cuda", 0)


def _extract(ex, imgs):
    """orbx_extract_batch_device on a torch stream: (desc [B, cap, 32], counts [B, 2]) tensors left in HBM, and the stream."""
    B, H, W = imgs.shape
    cap = ex.capacity
    s = torch.cuda.Stream(device=_dev())
    t = torch.from_numpy(np.ascontiguousarray(imgs)).to(_dev())
    kps = torch.zeros((B, cap, 28), dtype=torch.uint8, device=_dev())
    desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device=_dev())
    counts = torch.zeros((B, 2), dtype=torch.int32, device=_dev())
    torch.cuda.synchronize()
    ex.extract_batch_device(t.data_ptr(), B, H, W, W, H * W, kps.data_ptr(), desc.data_ptr(), counts.data_ptr(), (0, 1000), stream=s.cuda_stream)
    s.synchronize()
    return desc, counts, s, t


def _same(got, want, where):
    assert got is not None, where
    (gi, gv), gfv = got
    (wi, wv), wfv = want
    assert np.array_equal(gi, wi), where
    assert gv.tobytes() == wv.tobytes(), where
    assert gfv == wfv, where
    assert list(gfv) == sorted(gfv) and all(v == sorted(v) for v in gfv.values()), where


def _run(bb, desc, counts, stream, cap=None):
    B = desc.shape[0]
    out = bb.transform_device(desc, counts, B, desc.shape[1] if cap is None else cap, stream=stream.cuda_stream)
    stream.synchronize()
    return out


@pytest.fixture(scope="module")
def euroc():
    ex = ORBextractor(*EUROC[2], device_id=0)
    imgs = synth.make_stream(256, EUROC[0], EUROC[1])
    desc, counts, s, t = _extract(ex, imgs)
    hd, hc = desc.cpu().numpy(), counts.cpu().numpy()
    assert (hc[:, 0] > 800).all()
    return ex, imgs, desc, counts, s, hd, hc


def _voc(ex, tmp_path, train, k, L, scoring=None, weighting=None, name="voc.txt"):
    p = str(tmp_path / name)
    make_vocabulary(p, train, k, L, seed=10 * k + L)
    if scoring is not None:
        lines = open(p).read().split("\n")
        lines[0] = f"{k} {L} {scoring} {weighting}"
        open(p, "w").write("\n".join(lines))
    gv = ORBVocabulary(ex)
    assert gv.loadFromTextFile(p)
    return gv, po.OracleVocabulary(p), p


@pytest.mark.parametrize("k,L", [(10, 3), (10, 6), (3, 7), (20, 2)])
def test_parity_per_frame(euroc, tmp_path, k, L):
    ex, imgs, desc, counts, s, hd, hc = euroc
    train = np.concatenate([hd[f, :hc[f, 0]] for f in range(4)])
    gv, ov, _ = _voc(ex, tmp_path, train, k, L)
    # the inputs exercise what the test is about
    multi = dropped = once = 0
    for f in range(4):
        word, weight, _ = gv.descend(hd[f, :hc[f, 0]], 4)
        kept = word[weight > 0]
        hits = np.bincount(kept)
        multi += int(hits.max() >= 3)
        once += int((hits == 1).any())
        dropped += int((~(weight > 0)).any())
    if (k, L) == (10, 3):
        assert multi >= 1 and dropped >= 1, (multi, dropped)
    if (k, L) == (10, 6):
        assert once >= 1
    ex2 = ORBextractor(*VGA15[2], device_id=0)
    d2, c2, s2, _ = _extract(ex2, synth.make_stream(3, VGA15[0], VGA15[1], 77))
    hd2, hc2 = d2.cpu().numpy(), c2.cpu().numpy()
    assert ex2.capacity != ex.capacity and (hc2[:, 0] > 1000).all()
    sample = sorted({0, 255} | set(range(7, 256, 15)))
    assert len(sample) >= 18
    for levelsup in (0, 2, 4, L, L + 1):
        bb = BowBatch(gv, levelsup)
        want = {}

        def expect(f):
            if f not in want:
                d = hd[f, :hc[f, 0]]
                o, g = ov.transform(d, levelsup), gv.transform(d, levelsup)
                _same(g, o, ("single vs oracle", f))
                want[f] = o
            return want[f]

        for B in (1, 3, 12):
            res = _run(bb, desc[:B], counts[:B], s).frames()
            for f in range(B):
                _same(res[f], expect(f), (k, L, levelsup, B, f))
        res = _run(bb, desc, counts, s).frames(sample)
        for f, r in zip(sample, res):
            _same(r, expect(f), (k, L, levelsup, 256, f))
        res = _run(bb, d2, c2, s2).frames()
        for f in range(3):
            _same(res[f], ov.transform(hd2[f, :hc2[f, 0]], levelsup), (k, L, levelsup, "vga", f))
        if L - levelsup <= 0:
            assert all(set(r[1]) == {0} for r in res)
        bb.close()


def test_host_form_equals_device_form(euroc, tmp_path):
    ex, imgs, desc, counts, s, hd, hc = euroc
    gv, ov, _ = _voc(ex, tmp_path, np.concatenate([hd[f, :hc[f, 0]] for f in range(4)]), 10, 4)
    bb = BowBatch(gv, 2)
    got = bb.transform(hd[:7], hc[:7])
    got1 = bb.transform(hd[:7], hc[:7, 0])
    for f in range(7):
        _same(got[f], ov.transform(hd[f, :hc[f, 0]], 2), f)
        _same(got1[f], got[f], f)


@pytest.mark.parametrize("weighting", [TF_IDF, TF, IDF, BINARY])
@pytest.mark.parametrize("scoring", [0, 1, 2, 3, 4, 5])
def test_every_weighting_and_scoring(euroc, tmp_path, weighting, scoring):
    ex, imgs, desc, counts, s, hd, hc = euroc
    gv, ov, _ = _voc(ex, tmp_path, np.concatenate([hd[f, :hc[f, 0]] for f in range(2)]), 8, 2, scoring, weighting)
    bb = BowBatch(gv, 1)
    res = _run(bb, desc[:5], counts[:5], s).frames()
    for f in range(5):
        d = hd[f, :hc[f, 0]]
        single = gv.transform(d, 1)                       # orbx_bow_transform + orbx_bow_finalize
        assert max(np.bincount(single[0][0])) == 1 and len(single[0][0]) < hc[f, 0] - 100   # words are shared by many features
        _same(res[f], single, (weighting, scoring, f))
        _same(res[f], ov.transform(d, 1), (weighting, scoring, f, "oracle"))


def test_edges(tmp_path):
    H, W, params = 240, 320, (301, 1.2, 4, 20, 7)
    ex = ORBextractor(*params, device_id=0)
    cap = ex.capacity
    assert cap % 4 != 0 and cap % 64 != 0
    imgs = synth.make_stream(5, H, W, 31)
    imgs[1] = 128                                          # a constant image: count 0
    desc, counts, s, _ = _extract(ex, imgs)
    hd, hc = desc.cpu().numpy().copy(), counts.cpu().numpy().copy()
    assert hc[1, 0] == 0 and hc[0, 0] > 200
    gv, ov, _ = _voc(ex, tmp_path, hd[0, :hc[0, 0]], 6, 3)
    # frame 3 uses the full capacity (rows of other frames fill it up), frame 2 is marked as overflowed
    fill = np.concatenate([hd[f, :hc[f, 0]] for f in (0, 4)])
    reps = -(-cap // len(fill))
    hd[3] = np.concatenate([fill] * reps)[:cap]
    hc[3, 0] = cap
    hc[2, 0] = -1
    rng = np.random.default_rng(5)
    bb = BowBatch(gv, 1)
    results = []
    for fillbyte in (None, 0xFF, "random"):
        d = hd.copy()
        for f in range(5):
            n = max(int(hc[f, 0]), 0)
            if fillbyte == 0xFF:
                d[f, n:] = 0xFF
            elif fillbyte == "random":
                d[f, n:] = rng.integers(0, 256, d[f, n:].shape, dtype=np.uint8)
        td, tc = torch.from_numpy(d).to(_dev()), torch.from_numpy(hc).to(_dev())
        out = bb.transform_device(td, tc, 5, cap, stream=s.cuda_stream)
        s.synchronize()
        results.append((out.frames(), out.bow_n.cpu().numpy(), out.fv_n.cpu().numpy()))
    for res, bn, fn in results:
        assert bn[1] == 0 and fn[1] == 0 and res[1][1] == {} and len(res[1][0][0]) == 0 and len(res[1][0][1]) == 0
        assert bn[2] == -1 and fn[2] == -1 and res[2] is None
        for f in (0, 3, 4):
            _same(res[f], ov.transform(hd[f, :hc[f, 0]], 1), f)
            _same(res[f], gv.transform(hd[f, :hc[f, 0]], 1), f)
        assert bn[3] > 50
    # the overflow marker touches nothing else of its frame
    td, tc = torch.from_numpy(hd).to(_dev()), torch.from_numpy(hc).to(_dev())
    out = bb.transform_device(td, tc, 5, cap, stream=s.cuda_stream)
    s.synchronize()
    for t in (out.bow_ids, out.bow_vals, out.fv_node, out.fv_ptr, out.fv_feat):
        t[2] = 0 if t.dtype != torch.float64 else 7.0
    keep = [t[2].clone() for t in (out.bow_ids, out.bow_vals, out.fv_node, out.fv_ptr, out.fv_feat)]
    bb.transform_device(td, tc, 5, cap, out=out, stream=s.cuda_stream)
    s.synchronize()
    for t, k in zip((out.bow_ids, out.bow_vals, out.fv_node, out.fv_ptr, out.fv_feat), keep):
        assert torch.equal(t[2], k)
    # either output group alone
    only_b = bb.transform_device(td, tc, 5, cap, stream=s.cuda_stream, fv=False)
    only_f = bb.transform_device(td, tc, 5, cap, stream=s.cuda_stream, bow=False)
    s.synchronize()
    assert torch.equal(only_b.bow_n, out.bow_n) and torch.equal(only_f.fv_n, out.fv_n)
    n0 = int(out.bow_n[0])
    assert only_b.bow_vals[0, :n0].cpu().numpy().tobytes() == out.bow_vals[0, :n0].cpu().numpy().tobytes()
    m0 = int(out.fv_n[0])
    assert torch.equal(only_f.fv_ptr[0, :m0 + 1], out.fv_ptr[0, :m0 + 1]) and torch.equal(only_f.fv_node[0, :m0], out.fv_node[0, :m0])
    # invalid arguments: ORBX_E_INVALID with a reason
    Bl = _lib.bow_lib()
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    o = out
    good = [p(td), p(tc), 5, cap, p(o.bow_ids), p(o.bow_vals), p(o.bow_n), p(o.fv_node), p(o.fv_ptr), p(o.fv_feat), p(o.fv_n), None]
    for idx, bad in ((2, 0), (2, -3), (3, 0), (0, None), (1, None), (4, None), (9, None)):
        a = list(good)
        a[idx] = bad
        assert Bl.orbx_bow_transform_batch_device(bb._h, *a) == _lib.ORBX_E_INVALID, (idx, bad)
        assert len(Bl.orbx_bow_last_error(bb._h)) > 10
    a = list(good)
    a[4:11] = [None] * 7
    assert Bl.orbx_bow_transform_batch_device(bb._h, *a) == _lib.ORBX_E_INVALID and b"null outputs" in Bl.orbx_bow_last_error(bb._h)
    with pytest.raises(OrbxError):
        BowBatch(gv, -1)
    assert b"levelsup" in Bl.orbx_bow_last_error(None)
    empty = tmp_path / "empty.txt"
    empty.write_text("10 3 0 0")
    ev = ORBVocabulary(ex)
    if ev.loadFromTextFile(str(empty)):
        with pytest.raises(OrbxError):
            BowBatch(ev, 4)
        assert b"empty" in Bl.orbx_bow_last_error(None)
    if torch.cuda.device_count() > 1:
        other = torch.zeros((5, cap, 32), dtype=torch.uint8, device=torch.device("cuda", 1))
        a = list(good)
        a[0] = p(other)
        assert Bl.orbx_bow_transform_batch_device(bb._h, *a) == _lib.ORBX_E_INVALID and b"device" in Bl.orbx_bow_last_error(bb._h)


def test_both_paths(euroc, tmp_path, monkeypatch):
    ex, imgs, desc, counts, s, hd, hc = euroc
    gv, ov, _ = _voc(ex, tmp_path, np.concatenate([hd[f, :hc[f, 0]] for f in range(4)]), 10, 3)
    default = BowBatch(gv, 2)
    ref = _run(default, desc[:12], counts[:12], s)
    for limit in ("0", "500"):
        monkeypatch.setenv("ORBX_BOW_LDS", limit)
        low = BowBatch(gv, 2)
        monkeypatch.delenv("ORBX_BOW_LDS")
        got = _run(low, desc[:12], counts[:12], s)
        a, b = ref.frames(), got.frames()
        for f in range(12):
            _same(b[f], a[f], (limit, f))
        for name in ("bow_n", "fv_n"):
            assert torch.equal(getattr(ref, name), getattr(got, name))
        for f in range(12):   # byte for byte, every specified slot
            k, m = int(ref.bow_n[f]), int(ref.fv_n[f])
            assert torch.equal(ref.bow_ids[f, :k], got.bow_ids[f, :k]) and torch.equal(ref.bow_vals[f, :k].view(torch.int64), got.bow_vals[f, :k].view(torch.int64))
            assert torch.equal(ref.fv_ptr[f, :m + 1], got.fv_ptr[f, :m + 1]) and torch.equal(ref.fv_node[f, :m], got.fv_node[f, :m])
            assert torch.equal(ref.fv_feat[f, :int(ref.fv_ptr[f, m])], got.fv_feat[f, :int(ref.fv_ptr[f, m])])
        low.close()
    # the mi.yaml shape: 20 000 features on one level go through the global-memory path by themselves
    ex20 = ORBextractor(20000, 1.2, 1, 20, 7, device_id=0)
    rng = np.random.default_rng(9)
    big = np.stack([rng.integers(0, 256, (600, 800), dtype=np.uint8), synth.make_stream(1, 600, 800, 3)[0]])
    d20, c20, s20, _ = _extract(ex20, big)
    h20, n20 = d20.cpu().numpy(), c20.cpu().numpy()
    assert n20[0, 0] > 4096, n20
    res = _run(default, d20, c20, s20).frames()
    for f in range(2):
        _same(res[f], gv.transform(h20[f, :n20[f, 0]], 2), ("mi", f))
    default.close()


def test_a_tree_that_leaves_l2(euroc, tmp_path):
    ex, imgs, desc, counts, s, hd, hc = euroc
    docs, trainer = [], ex.clone()
    for a in range(0, 1024, 64):
        docs += [r[2] for r in trainer.extract_batch(synth.make_stream(64, 480, 640, 9000 + a), (0, 1000))]
    assert sum(len(d) for d in docs) >= 10 ** 6 - 10 ** 5
    extra = [hd[f, :hc[f, 0]] for f in range(64, 200)]
    docs += extra
    assert sum(len(d) for d in docs) >= 10 ** 6
    gv = ORBVocabulary(ex)
    gv.create(docs, 10, 6, 0, 0, seed=2024)
    assert gv.info()["words"] >= 100_000
    bb = BowBatch(gv, 4)
    frames = [0, 9, 18, 27, 36, 45, 54, 63]
    res = _run(bb, desc[:64], counts[:64], s).frames(frames)
    rv = None
    if po.ref_available():
        txt = str(tmp_path / "big.txt")
        gv.saveToTextFile(txt)
        gv2 = ORBVocabulary(ex)            # the text format keeps 6 digits of each weight: compare on the tree the reference reads
        assert gv2.loadFromTextFile(txt)
        rv = po.RefVocabulary(txt)
        bb2 = BowBatch(gv2, 4)
        res2 = _run(bb2, desc[:64], counts[:64], s).frames(frames)
    for i, f in enumerate(frames):
        d = hd[f, :hc[f, 0]]
        _same(res[i], gv.transform(d, 4), f)
        if rv is not None:
            _same(res2[i], rv.transform(d, 4), ("ref", f))


def test_scores(euroc, tmp_path):
    ex, imgs, desc, counts, s, hd, hc = euroc
    gv, ov, _ = _voc(ex, tmp_path, np.concatenate([hd[f, :hc[f, 0]] for f in range(4)]), 10, 4)
    bb = BowBatch(gv, 4)
    cap = ex.capacity
    q = _run(bb, desc[:64], counts[:64], s)
    db = _run(BowBatch(gv, 4), desc[:150], counts[:150], s)
    db_ids, db_vals, db_n = torch.cat([db.bow_ids, db.bow_ids]), torch.cat([db.bow_vals, db.bow_vals]), torch.cat([db.bow_n, db.bow_n])
    db_n[299] = -1                                          # an overflowed frame scores as an empty vector
    db_n[298] = 0
    self_m = bb.score_matrix_device(q.bow_ids, q.bow_vals, q.bow_n, 64, cap, q.bow_ids, q.bow_vals, q.bow_n, 64, cap, stream=s.cuda_stream)
    cross = bb.score_matrix_device(q.bow_ids, q.bow_vals, q.bow_n, 64, cap, db_ids, db_vals, db_n, 300, cap, stream=s.cuda_stream)
    s.synchronize()
    self_m, cross = self_m.cpu().numpy(), cross.cpu().numpy()
    qv = [r[0] for r in q.frames()]
    dv = [r[0] for r in db.frames()]
    dv = dv + dv
    dv[298] = dv[299] = (np.zeros(0, np.uint32), np.zeros(0, np.float64))
    want_self = np.array([[gv.score(a, b) for b in qv] for a in qv])
    want_cross = np.array([[gv.score(a, b) for b in dv] for a in qv])
    assert self_m.tobytes() == want_self.tobytes()
    assert cross.tobytes() == want_cross.tobytes()
    assert (cross[:, 298:] == 0).all() and (np.diag(self_m) > 0.999).all()
    for i in (0, 31, 63):
        assert gv.score_batch(qv[i], qv)[i].tobytes() == self_m[i, i].tobytes()
        assert want_self[i, (i + 1) % 64] == po.score_l1(qv[i], qv[(i + 1) % 64])
    # the host form
    host = bb.score_matrix(qv[:9], dv[:40] + dv[298:])
    assert host.tobytes() == want_cross[:9, list(range(40)) + [298, 299]].tobytes()
    # a vocabulary whose vectors carry another norm is rejected
    gl2, _, _ = _voc(ex, tmp_path, hd[0, :hc[0, 0]], 6, 2, L2_NORM, TF, name="l2.txt")
    bl2 = BowBatch(gl2, 1)
    with pytest.raises(OrbxError) as ei:
        bl2.score_matrix_device(q.bow_ids, q.bow_vals, q.bow_n, 64, cap, q.bow_ids, q.bow_vals, q.bow_n, 64, cap, stream=s.cuda_stream)
    assert ei.value.code == _lib.ORBX_E_INVALID and "L1" in str(ei.value)
    with pytest.raises(OrbxError):
        bl2.score_matrix(qv[:2], qv[:2])
    gdot, _, _ = _voc(ex, tmp_path, hd[0, :hc[0, 0]], 6, 2, DOT_PRODUCT, TF_IDF, name="dot.txt")
    with pytest.raises(OrbxError):
        BowBatch(gdot, 1).score_matrix(qv[:2], qv[:2])


def test_from_a_replay_block(euroc, tmp_path):
    from orb_slam3_modified_amd.replay import ReplayEngine
    ex, imgs, desc, counts, s, hd, hc = euroc
    gv, ov, _ = _voc(ex, tmp_path, np.concatenate([hd[f, :hc[f, 0]] for f in range(4)]), 10, 4)
    B = 32
    frames = torch.from_numpy(imgs[:B]).to(_dev())
    ex2 = ex.clone()
    eng = ReplayEngine(ex2, frames, lapping=(0, 1000), gather=True, lanes=1, gather_what="descriptors")
    assert eng.world == 1 and eng.layout.cap == ex.capacity and eng.send_off == eng.layout.desc_off
    i = eng.step()
    cons = torch.cuda.Stream(device=_dev())
    eng.wait_gathered(i, cons.cuda_stream)                  # the consumer's work waits for this step's exchange, on the device
    part = eng.gathered_ptr(i, 0)
    bb = BowBatch(gv, 4)
    out = bb.transform_device(part, part + (eng.layout.counts_off - eng.layout.desc_off), B, eng.layout.cap, stream=cons.cuda_stream)
    eng.release_gathered(i, cons.cuda_stream)
    cons.synchronize()
    own = _run(bb, desc[:B], counts[:B], s)
    a, b = out.frames(), own.frames()
    for f in range(B):
        _same(a[f], b[f], f)
        _same(a[f], ov.transform(hd[f, :hc[f, 0]], 4), f)
    # the block itself, through orbx_replay_layout's offsets
    eng.drain()
    blk = eng.block_ptr(i)
    out2 = bb.transform_device(blk + eng.layout.desc_off, blk + eng.layout.counts_off, B, eng.layout.cap, stream=cons.cuda_stream)
    cons.synchronize()
    for f, r in enumerate(out2.frames()):
        _same(r, b[f], f)
    eng.close()


def test_lifetimes(tmp_path):
    ex = ORBextractor(500, 1.2, 6, 20, 7, device_id=0)
    imgs = synth.make_stream(6, 240, 320, 12)
    desc, counts, s, _ = _extract(ex, imgs)
    hd, hc = desc.cpu().numpy(), counts.cpu().numpy()
    gv, ov, _ = _voc(ex, tmp_path, hd[0, :hc[0, 0]], 7, 3)
    single = ex.clone()

    def one_frame():
        d = np.ascontiguousarray(single(imgs[2], None, (0, 1000))[2])
        single.publish_descriptors(d)
        pub = gv.descend_published(d, 4)
        return gv.transform(d, 4), pub

    before, _ = one_frame()
    a, b = BowBatch(gv, 4), BowBatch(gv, 2)
    want4 = [ov.transform(hd[f, :hc[f, 0]], 4) for f in range(6)]
    want2 = [ov.transform(hd[f, :hc[f, 0]], 2) for f in range(6)]
    for _ in range(3):                                      # two handles on one vocabulary, alternately
        ra = a.transform_device(desc, counts, 6, ex.capacity, stream=s.cuda_stream)
        rb = b.transform_device(desc, counts, 6, ex.capacity, stream=s.cuda_stream)
        s.synchronize()
        for f in range(6):
            _same(ra.frames()[f], want4[f], f)
            _same(rb.frames()[f], want2[f], f)
    after, pub = one_frame()
    _same(after, before, "single frame after a batch")
    assert pub is not None and np.array_equal(pub[0], gv.descend(np.ascontiguousarray(single(imgs[2], None, (0, 1000))[2]), 4)[0])
    ra = a.transform_device(desc, counts, 6, ex.capacity)   # the handle's own stream, work still in flight at destruction
    a.close()
    b.close()
    a.close()                                               # the handle goes before the vocabulary and the context
    _same(gv.transform(hd[1, :hc[1, 0]], 4), want4[1], "vocabulary after its handles")
    del gv
    gc.collect()
    okps, odesc, omono = po.OracleExtractor(500, 1.2, 6, 20, 7).extract(imgs[0], (0, 1000))
    r = ex(imgs[0], None, (0, 1000))
    assert r[0] == omono and r[1].tobytes() == okps.tobytes() and np.array_equal(r[2], odesc)
