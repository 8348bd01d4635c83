"""The constructed cases of tests/bow_edge_cases.py are what they claim to be, by the oracle alone: a case that misses its edge fails here and
not silently on the GPU (tests/test_gpu_bow_batch_edges.py runs the same cases)."""
import math

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import bow_edge_cases as bc


def test_the_limits_are_the_source_s():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "orb_slam3_modified_amd", "csrc", "bow", "orbx_bow.hip")).read()
    assert int(re.search(r"constexpr int kBowLds = (\d+);", src).group(1)) == bc.KEY_LDS
    assert int(re.search(r"constexpr int kScoreLds = (\d+);", src).group(1)) == bc.QUERY_LDS
    assert 'env_int("ORBX_BOW_LDS", 0, kBowLds, kBowLds)' in src
    assert f"ORBX_BOW_LDS (0 .. {bc.KEY_LDS})" in open(os.path.join(root, "include", "orbx_bow.h")).read()
    assert bc.CAP >= 4200 and bc.CAP > bc.KEY_LDS + 1 and bc.CAP % 4 != 0 and bc.CAP % 64 != 0
    assert bc.Q_CAP != bc.DB_CAP and bc.Q_CAP > bc.QUERY_LDS + 1


@pytest.fixture(scope="module", params=sorted(bc.TREES))
def tree(request, tmp_path_factory):
    path = bc.vocabulary_file(str(tmp_path_factory.mktemp("voc") / f"{request.param}.txt"), request.param)
    return request.param, path, po.OracleVocabulary(path), bc.transform_frames(path)


def test_vocabularies(tree):
    name, path, ov, frames = tree
    t = bc.TREES[name]
    assert 4 <= t["k"] <= 10 and 2 <= t["L"] <= 3
    leaves = bc.leaf_descriptors(path)
    assert 10 <= len(leaves) <= 300
    word, weight, _ = ov.descend(np.concatenate([bc.pool(), leaves]), 0)
    zero = np.unique(word[~(weight > 0)])
    assert len(np.unique(word)) == len(leaves)                     # every word is reached
    assert 3 <= len(zero) <= len(leaves) // 4, zero               # several words weigh exactly 0, most do not
    assert (weight[~(weight > 0)] == 0).all()
    if t["weights"] == "idf":                                      # ... and by DBoW2's rule: log(N / Ni) with Ni = N
        pos = np.unique(weight[weight > 0])
        assert len(zero) >= bc.STOP_WORDS and len(pos) > 5
        assert all(any(w == math.log(bc.DOCS / ni) for ni in range(1, bc.DOCS)) for w in pos)
    print(f"{name}: {len(leaves)} words, {len(zero)} of weight 0")


def test_transform_frames(tree):
    name, path, ov, frames = tree
    levelsup = bc.TREES[name]["levelsup"]
    by = {f.name: f for f in frames}
    assert len(by) == len(frames) <= 24
    nwords = len(bc.leaf_descriptors(path))
    seen_kept = set()
    for f in frames:
        if f.rows is None:
            continue
        assert f.rows.shape == (len(f.rows), 32) and len(f.rows) <= bc.CAP
        word, weight, node = ov.descend(f.rows, levelsup)
        kept = weight > 0
        assert int(kept.sum()) == f.kept, f.name                   # the number of keys is the intended one
        (ids, vals), fv = ov.transform(f.rows, levelsup)
        assert len(ids) == len(np.unique(word[kept])) and sum(len(v) for v in fv.values()) == f.kept
        if f.zero is not None:                                     # the weight-0 features are exactly the stated rows, and they are lost
            assert np.array_equal(np.flatnonzero(~kept), f.zero), f.name
            assert not set(f.zero.tolist()) & {i for v in fv.values() for i in v}
        if f.name.startswith("kept"):
            assert f.name == f"kept{f.kept}"
            seen_kept.add(f.kept)
            assert len(f.rows) == f.kept or f.kept < bc.KEY_LDS - 1
            assert f.kept < 60 or len(ids) > 10                    # many runs
        print(f"{name}/{f.name}: count {len(f.rows)}, kept {f.kept}, words {len(ids)}, nodes {len(fv)}")
    assert seen_kept == set(bc.KEPT_COUNTS) == {0, 1, 2, 3, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, bc.CAP}
    for n in (bc.KEY_LDS, bc.KEY_LDS + 1):                         # one word holds every feature: one run of n
        f = by[f"oneword{n}"]
        word, weight, _ = ov.descend(f.rows, levelsup)
        assert len(f.rows) == n == f.kept and len(np.unique(word)) == 1 and weight[0] > 0
        assert len(np.unique(f.rows, axis=0)) > 1                  # ... of different descriptors
    f = by["everyword"]                                            # every feature its own word, every word once, not in word order
    word, weight, _ = ov.descend(f.rows, levelsup)
    assert len(f.rows) == nwords and np.array_equal(np.sort(word), np.arange(nwords)) and not np.array_equal(word, np.sort(word))
    assert f.kept == len(ov.transform(f.rows, levelsup)[0][0]) > nwords // 2
    assert by["allzero"].kept == 0 and len(by["allzero"].rows) > 64 and len(ov.transform(by["allzero"].rows, levelsup)[0][0]) == 0
    assert by["allbutone"].kept == 1 and len(by["allbutone"].zero) == len(by["allbutone"].rows) - 1 > 64
    f = by["zerofirst64"]
    assert np.array_equal(f.zero, np.arange(64)) and f.kept == bc.KEY_LDS and len(f.rows) == bc.KEY_LDS + 64
    f = by["zerolast64"]
    assert np.array_equal(f.zero, np.arange(len(f.rows) - 64, len(f.rows))) and len(f.rows) % 64 == 0 and 512 < len(f.rows) <= bc.KEY_LDS
    i = [f.name for f in frames].index("overflow")                 # the count -1 lies between two large frames
    assert by["overflow"].rows is None and len(frames[i - 1].rows) > bc.KEY_LDS and len(frames[i + 1].rows) == bc.CAP


def test_transform_batch(tree):
    name, path, ov, frames = tree
    batches = [bc.transform_batch(frames, v) for v in (0, 1)]
    for v, (desc, counts) in enumerate(batches):
        assert desc.shape == (len(frames), bc.CAP, 32) and desc.dtype == np.uint8 and counts.shape == (len(frames), 2) and counts.dtype == np.int32
        for f, fr in enumerate(frames):
            n = counts[f, 0]
            assert n == (-1 if fr.rows is None else len(fr.rows))
            if n > 0:
                assert np.array_equal(desc[f, :n], fr.rows)
            tail = desc[f, max(n, 0):]
            if len(tail):
                assert (tail == 0xFF).all() == ((f + v) % 2 == 0)
                assert (tail == 0xFF).all() or len(np.unique(tail)) > 200
    assert np.array_equal(batches[0][1], batches[1][1])
    assert np.array_equal(bc.transform_batch(frames, 0)[0], batches[0][0])   # deterministic
    again = bc.transform_frames(path)
    assert all(a.rows is b.rows or np.array_equal(a.rows, b.rows) for a, b in zip(frames, again))


@pytest.fixture(scope="module")
def scores():
    cases = bc.score_cases()
    return cases, bc.expected_scores(cases)


def test_score_vectors(scores):
    cases, want = scores
    assert len(cases.q) == bc.NQ and len(cases.db) == bc.NDB
    assert [len(a) for a, _ in cases.q[:-1]] == [0, 1, 3999, 4000, 4001, 8192] == list(bc.QUERY_LENGTHS[:-1]) and bc.QUERY_LENGTHS[-1] == -1
    assert len(cases.q[5][0]) == bc.Q_CAP
    dl = [len(a) for a, _ in cases.db]
    assert {0, 1, 4001, 8192} <= set(dl) and sum(100 <= n <= 700 for n in dl) > 400 and max(dl) < bc.DB_CAP
    for ids, vals in cases.q + cases.db:
        assert ids.dtype == np.uint32 and vals.dtype == np.float64 and len(ids) == len(vals)
        assert (np.diff(ids.astype(np.int64)) > 0).all() and (vals > 0).all()
        if len(ids):
            s = 0.0
            for v in vals:                                         # the running sum BowVector::normalize takes
                s += v
            assert abs(s - 1.0) < 1e-12
    ids = np.concatenate([a for a, _ in cases.q + cases.db])
    assert ids.min() == 0 and ids.max() == bc.TOP_ID == 2 ** 32 - 1
    for side in (cases.q, cases.db):
        assert any(len(a) and a[0] == 0 for a, _ in side) and any(len(a) and a[-1] == bc.TOP_ID for a, _ in side)
    assert {(nq, ndb) for nq, ndb in bc.SHAPES} == {(a, b) for a in (1, 7) for b in (1, 255, 256, 257, 513)}
    qi, qv, qn = bc.fixed_stride(cases.q, bc.Q_CAP, {bc.NQ - 1}, 1)
    assert qn.tolist() == list(bc.QUERY_LENGTHS) and qi.shape == (bc.NQ, bc.Q_CAP)
    di, dv, dn = bc.fixed_stride(cases.db, bc.DB_CAP, {bc.DB_OVERFLOW}, 2)
    assert dn[bc.DB_OVERFLOW] == -1 and len(cases.db[bc.DB_OVERFLOW][0]) > 50 and (want[2:6, bc.DB_OVERFLOW] == 0).all()
    assert po.score_l1(cases.q[5], cases.db[bc.DB_OVERFLOW]) > 0       # ... which its entries would not give
    # the slots past a count would change the scores if they were read
    full = (qi[4], qv[4])
    assert np.array_equal(qi[4, :bc.QUERY_LDS + 1], cases.q[4][0]) and qn[4] < bc.Q_CAP and (np.diff(qi[4, qn[4]:].astype(np.int64)) >= 0).all()
    assert len(np.intersect1d(full[0][qn[4]:], np.concatenate([a for a, _ in cases.db[20:60]]))) > 100


def test_score_patterns(scores):
    cases, want = scores
    q, db = cases.q, cases.db
    p = cases.patterns
    assert set(p) == {"identical", "disjoint", "interleaved", "first", "last", "long_vs_one", "one_vs_long", "extreme_ids", "empty"}
    common = lambda qi, di: np.intersect1d(q[qi][0], db[di][0])   # noqa: E731
    for qi, di in p["identical"]:
        assert np.array_equal(q[qi][0], db[di][0]) and q[qi][1].tobytes() == db[di][1].tobytes() and abs(want[qi, di] - 1) < 1e-12
    assert any(want[qi, di] == 1.0 for qi, di in p["identical"])
    for qi, di in p["disjoint"]:
        assert db[di][0].min() > q[qi][0].max() and want[qi, di] == 0
    for qi, di in p["interleaved"]:
        a, b = q[qi][0], db[di][0]
        assert len(common(qi, di)) == 0 and want[qi, di] == 0
        assert min(len(a), len(b)) > 3000 and a[0] < b[-1] and b[0] < a[-1]
        merged = np.argsort(np.concatenate([a, b]), kind="stable") >= len(a)     # the merge changes sides thousands of times
        assert np.count_nonzero(np.diff(merged.astype(np.int8))) > 2000
    for qi, di in p["first"]:
        c = common(qi, di)
        assert len(c) == 1 and c[0] == q[qi][0][0] == db[di][0][0] and 0 < want[qi, di] < 1
    for qi, di in p["last"]:
        c = common(qi, di)
        assert len(c) == 1 and c[0] == q[qi][0][-1] == db[di][0][-1] and 0 < want[qi, di] < 1
    for qi, di in p["long_vs_one"]:
        assert len(q[qi][0]) > bc.QUERY_LDS and len(db[di][0]) == 1 and 0 < want[qi, di] < 1
    for qi, di in p["one_vs_long"]:
        assert len(q[qi][0]) == 1 and len(db[di][0]) == 8192 and 0 < want[qi, di] < 1
    for qi, di in p["extreme_ids"]:
        assert bc.TOP_ID in common(qi, di) and 0 < want[qi, di] < 1
    assert any(0 in common(qi, di) for qi, di in p["extreme_ids"])
    # the patterns reach the query in LDS and the query in global memory
    staged = {name for name, v in p.items() for qi, _ in v if len(q[qi][0]) <= bc.QUERY_LDS}
    beyond = {name for name, v in p.items() for qi, _ in v if len(q[qi][0]) > bc.QUERY_LDS}
    assert staged >= {"identical", "disjoint", "interleaved", "extreme_ids"} and beyond == set(p) - {"one_vs_long"}
    # the first database vector, which is all a one-column matrix holds, is a long one
    assert len(db[0][0]) == 8192 and (want[1:6, 0] > 0).all()
    assert all(len(db[i][0]) >= 100 and (want[2:6, i] > 0).all() for i in (254, 255, 256, 257, 512))


def test_expected_scores(scores):
    cases, want = scores
    assert want.shape == (bc.NQ, bc.NDB) and np.isfinite(want).all()
    zero, one = int((want == 0).sum()), int((want == 1).sum())
    between = int(((want > 0) & (want < 1)).sum())
    print(f"expected scores: {want.size} pairs, {zero} exactly 0, {one} exactly 1, {between} strictly between 0 and 1, maximum {want.max()!r}")
    assert zero >= 1 and one >= 1 and 2 * between > want.size
    assert (want[0] == 0).all() and (want[bc.NQ - 1] == 0).all()   # the empty query and the overflowed one
    assert (want >= 0).all() and want.max() < 1 + 1e-12
    assert len(np.unique(want)) > want.size // 2
