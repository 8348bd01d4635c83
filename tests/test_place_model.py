"""tests/place_model.py, the specification of the batched place recognition, held to the reference in two ways (CPU only): its steps 1-4
to oracle.pyoracle's mo_kfdb_query on every constructed world of tests/place_cases.py, and the whole routine to the results the
reference's own src/KeyFrameDatabase.cc recorded in tests/golden/kfdb_world_ref.txt.gz for the reloc_* and nbest_* calls of
tests/support/kfdb_world.cpp, whose keyframe graph is rebuilt here from the same golden world and vocabulary.  Each planted world is
shown to depend on its rule."""
import gzip
import os
import struct

import numpy as np
import pytest

from tests import place_cases as pc
from tests import place_model as pm
from tests import world_util as wu

WORLDS = list(pc.planted().values()) + [pc.size_edge(D, Q) for D, Q in pc.SIZE_EDGES]


@pytest.mark.parametrize("w", WORLDS, ids=lambda w: w["name"])
def test_opening_equals_the_oracle(w):
    from oracle import pyoracle as po
    odb = po.OracleKeyFrameDatabase()
    for d, row in enumerate(w["db"]):
        if row is not None:
            odb.add(d, row)
    some = 0
    for kind in (pm.RELOC, pm.NBEST):
        for q, ex in zip(w["q"], w["excl"]):
            ex = ex if kind == pm.NBEST else []
            want, got = odb.query(q, ex), pm.opening(q, w["db"], ex)
            assert got["rows"] == want["kf"].tolist() and got["words"] == want["words"].tolist()
            assert (got["max_common"], got["min_common"]) == (want["max_common"], want["min_common"])
            assert got["scored"] == (want["score"] != -1.0).tolist()
            si = np.array([s for s in got["si"] if s is not None], np.float32)
            assert np.array_equal(si.view(np.uint32), want["score"][want["score"] != -1.0].astype(np.float32).view(np.uint32))
            some += len(si)
    assert some > 0


@pytest.mark.parametrize("w", list(pc.planted().values()), ids=lambda w: w["name"])
def test_each_planted_world_depends_on_its_rule(w):
    for rule in w["rule"]:
        assert rule in pm.DROPS
        assert any(not pc.same(pc.run_model(kind, w), pc.run_model(kind, w, drop=rule)) for kind in w["kinds"]), rule


def test_what_the_planted_worlds_claim():
    p = pc.planted()
    r = pc.run_model(pm.RELOC, p["unscored_neighbour_in"])
    assert r["cand"][0, :2].tolist() == [1, -1] and r["stats"][0].tolist() == [3, 2, 10, 8]
    r = pc.run_model(pm.RELOC, p["unscored_neighbour_earlier_query"])
    assert r["cand"][1, :2].tolist() == [1, -1] and r["score"][1] == np.float32(5.0)
    w = p["equal_acc_and_first_word"]
    assert pc.run_model(pm.RELOC, w)["cand"][0, :6].tolist() == [4, 0, 1, 2, 3, -1]
    assert pc.run_model(pm.NBEST, w)["cand"][0, :3].tolist() == [4, 0, -1]                    # acc 8/16 five times: list order
    assert pc.run_model(pm.RELOC, p["truncation_5_10_15"])["stats"].tolist() == [[2, 1, 5, 4], [3, 2, 10, 8], [3, 2, 15, 12]]
    w = p["holder_twice_and_other_map_first"]
    assert pc.run_model(pm.RELOC, w)["cand"][0, :2].tolist() == [2, -1]
    r = pc.run_model(pm.NBEST, w)
    assert r["cand"][0, :2].tolist() == [2, -1] and r["merge"][0, :2].tolist() == [4, -1]
    w = p["ccap_below_count"]
    r = pc.run_model(pm.RELOC, w)
    assert r["ncand"][0] == 6 and r["cand"][0].tolist() == [0, 1, 2]
    r = pc.run_model(pm.NBEST, w)
    assert (r["ncand"][0], r["nmerge"][0]) == (5, 5) and r["cand"][0].tolist() == [0, 1, 2] and r["merge"][0].tolist() == [6, 7, 8]
    w = p["empty_erased_excluded"]
    r = pc.run_model(pm.NBEST, w)
    assert r["ncand"].tolist() == [0, 0, 2] and r["stats"][:2].tolist() == [[0, 0, 0, 0]] * 2 and r["stats"][2, 0] == 2
    assert pc.run_model(pm.RELOC, w)["stats"][:, 0].tolist() == [0, 2, 3]
    w = p["cov_padding_and_self"]
    assert pc.run_model(pm.NBEST, w)["cand"][0, :2].tolist() == [0, 1] and pc.run_model(pm.RELOC, w)["cand"][0, :2].tolist() == [0, -1]


# ---- the reference's recorded results ------------------------------------------------------------------------------------------------
NKF, QUERY_KFS = 64, (21, 45, 26)
MAP_OF = [0 if i < 40 else 1 if i < 54 else 2 for i in range(NKF)]
BAD_MAPS = (2,)


def _h(i, salt):
    """world_scene.h's H."""
    m = 0xFFFFFFFF
    x = (i * 2654435761 + salt * 40503 + 0x9e3779b9) & m
    x ^= x >> 15
    x = (x * 2246822519) & m
    x ^= x >> 13
    x = (x * 3266489917) & m
    x ^= x >> 16
    return x


def _views(path):
    """The descriptors of the world file's views (tests/world_util.py: write_world)."""
    b = open(path, "rb").read()
    magic, _, _, nlevels = struct.unpack_from("<iiii", b, 0)
    assert magic == 0x0b5e55ed
    o = 16 + 12 * nlevels + 8
    (nviews,), o = struct.unpack_from("<i", b, o), o + 4
    out = []
    for _ in range(nviews):
        (n,), o = struct.unpack_from("<i", b, o), o + 4
        o += 28 * n
        out.append(np.frombuffer(b, np.uint8, 32 * n, o).reshape(n, 32))
        o += 32 * n
        (npairs,), o = struct.unpack_from("<i", b, o), o + 4
        o += 8 * npairs
    assert o == len(b)
    return out


class _Graph:
    """kfdb_world.cpp's keyframes, covisibility and database, the database as rows in add() order."""

    def __init__(self, world):
        from oracle import pyoracle as po
        voc = po.OracleVocabulary(world + ".voc.txt")
        views = _views(world)
        nv = len(views)
        self.bow = []
        for i in range(NKF):
            desc = views[i % nv]
            m, start = 180 + _h(i, 1) % 160, 23 * (i // nv)
            rows = [(start + 2 * j + _h(j, 2 + i) % 2) % len(desc) for j in range(m)]
            self.bow.append(voc.transform(desc[rows], 2)[0])
        self.frame = voc.transform(views[1], 2)[0]
        self.ordered, self.connected = [], []
        for i in range(NKF):
            wts = []
            for d in (-16, -5, -3, -2, -1, 1, 2, 3, 5, 16, 20):
                j = i + d
                if j < 0 or j >= NKF or MAP_OF[j] != MAP_OF[i]:
                    continue
                wts.append((200 - 7 * abs(d) + _h(min(i, j) * 64 + max(i, j), 3) % 9, j))
            self.connected.append(sorted(j for _, j in wts))
            self.ordered.append([j for _, j in sorted(wts, key=lambda t: -t[0])])      # sorted is stable, as std::stable_sort
        self.rows, self.live = [], []    # row -> keyframe; an erased row keeps its place and its keyframe's fields
        for i in range(NKF):
            if i not in QUERY_KFS:
                self.add(i)

    def add(self, i):
        self.rows.append(i)
        self.live.append(True)

    def erase(self, i):
        self.live = [l and r != i for r, l in zip(self.rows, self.live)]

    def row_of(self):
        """keyframe -> its last row, erased or not"""
        return {kf: r for r, kf in enumerate(self.rows)}

    def arrays(self, fields, column):
        """(db, kf_map, kf_cov, kf_score) of the database as it stands, the score field seeded from a record's `fields`."""
        D, where = max(len(self.rows), 1), self.row_of()
        db = [self.bow[kf] if l else None for kf, l in zip(self.rows, self.live)] or [None]
        kf_map = np.array([MAP_OF[kf] for kf in self.rows] or [0], np.int32)
        cov = np.full((D, pm.COV), -1, np.int32)
        score = np.zeros(D, np.float32)
        for r, kf in enumerate(self.rows):
            if where[kf] == r:
                nb = [where.get(j, -1) for j in self.ordered[kf][:pm.COV]]
                cov[r, :len(nb)] = nb
                score[r] = np.array([fields[12 * kf + column]], np.uint32).view(np.float32)[0]
        return db, kf_map, cov, score


def _records(txt):
    out, name = [], None
    for l in txt.splitlines():
        if not l.startswith("  "):
            name = l.split()[0]
            out.append([name, {}])
        else:
            what, vals = l.strip().split(":")
            out[-1][1][what.split("[")[0]] = [int(v) for v in vals.split()]
    return out


@pytest.fixture(scope="module")
def recorded(tmp_path_factory):
    world = str(tmp_path_factory.mktemp("place") / "world.bin")
    wu.write_world(world)
    assert open(world, "rb").read() == gzip.open(os.path.join(wu.ROOT, "tests", "golden", "matcher_world.bin.gz")).read()
    recs = _records(gzip.open(os.path.join(wu.ROOT, "tests", "golden", "kfdb_world_ref.txt.gz")).read().decode())
    assert len(recs) == 24
    return _Graph(world), recs


# kfdb_world.cpp's sequence: a record's name, or what happens to the database between two records
SEQUENCE = [("reloc_mapA", 0), ("reloc_mapB", 1), "loop_minscore_0", "loop_minscore_hi", "candidates_0", "candidates_hi", "candidates_from_mapB",
            "best_minwords_0", "best_minwords_60", ("nbest_3", 21, 3), "nbest_3_same_id_again", ("nbest_10_from_mapB", 45, 10),
            ("erase", 22), ("erase", 23), ("erase", 37), ("erase", 50), ("reloc_after_erase", 0), ("nbest_after_erase", 21, 5),
            ("add", 23), ("add", 50), ("reloc_after_readd", 0), "candidates_after_readd", "best_after_readd", ("erase", 22), ("clearMap", 1),
            ("reloc_after_clearMap", 1), "candidates_after_clearMap", ("nbest_after_clearMap", 45, 4), ("clear",), ("reloc_after_clear", 0),
            ("nbest_after_clear", 21, 3), ("add", 3), ("add", 7), ("add", 11), ("add", 19), ("reloc_four_keyframes", 0), "best_four_keyframes"]
RELOC_COL, NBEST_COL = 11, 8             # mRelocScore, mPlaceRecognitionScore among a keyframe's twelve dumped fields


def _compare(g, rec, res, kind, qi, column):
    name, body = rec
    where = g.row_of()
    kf_of = lambda rows: [g.rows[r] + 1 for r in rows]   # noqa: E731
    if kind == pm.RELOC:
        assert kf_of(res["cand"][qi, :res["ncand"][qi]]) == body["candidates"], name
    else:
        assert kf_of(res["cand"][qi, :res["ncand"][qi]]) == body["loop"] and kf_of(res["merge"][qi, :res["nmerge"][qi]]) == body["merge"], name
    return where


def test_whole_routine_equals_the_reference_s_recorded_results(recorded):
    g, recs = recorded
    ri, before, checked, nonempty = 0, [0] * (12 * NKF), [], 0
    for step in SEQUENCE:
        if isinstance(step, str):
            assert recs[ri][0] == step
            before, ri = recs[ri][1]["fields"], ri + 1
            continue
        if step[0] in ("erase", "add"):
            getattr(g, step[0])(step[1])
            continue
        if step[0] == "clearMap":
            for i in range(NKF):
                if MAP_OF[i] == step[1]:
                    g.erase(i)
            continue
        if step[0] == "clear":
            g.live = [False] * len(g.rows)
            continue
        name, body = recs[ri]
        assert name == step[0]
        kind = pm.RELOC if name.startswith("reloc") else pm.NBEST
        column = RELOC_COL if kind == pm.RELOC else NBEST_COL
        db, kf_map, cov, score = g.arrays(before, column)
        where = g.row_of()
        if kind == pm.RELOC:
            res = pm.run(kind, db, kf_map, cov, score, [g.frame], [step[1]], ccap=NKF)
        else:
            ex = [[where[j] for j in g.connected[step[1]] if j in where]]
            # the driver asks with the same keyframe more than once: the rows that still carry its id from the earlier call
            marked = [[r for kf, r in where.items() if before[12 * kf + NBEST_COL - 2] == step[1] + 1]]
            res = pm.run(kind, db, kf_map, cov, score, [g.bow[step[1]]], [MAP_OF[step[1]]], ex, step[2], ccap=NKF, bad_maps=BAD_MAPS,
                         marked=marked)
        _compare(g, recs[ri], res, kind, 0, column)
        for kf, r in where.items():
            assert int(res["score"][r:r + 1].view(np.uint32)[0]) == body["fields"][12 * kf + column], (name, kf)
        nonempty += int(res["ncand"][0] > 0)
        checked.append(name)
        before, ri = body["fields"], ri + 1
    assert ri == 24 and len(checked) == 12 and "nbest_3_same_id_again" not in checked and nonempty >= 6


def test_the_adjacent_reloc_pair_as_one_call_of_two_queries(recorded):
    """reloc_mapA then reloc_mapB: query 1 finds the scores query 0 left, and the call's OUT array is the second record's."""
    g0, recs = recorded
    g = _Graph.__new__(_Graph)
    g.__dict__.update(g0.__dict__)
    g.rows = [i for i in range(NKF) if i not in QUERY_KFS]
    g.live = [True] * len(g.rows)
    assert recs[0][0] == "reloc_mapA" and recs[1][0] == "reloc_mapB"
    db, kf_map, cov, score = g.arrays([0] * (12 * NKF), RELOC_COL)       # the driver's KeyFrame starts with mRelocScore = 0
    res = pm.run(pm.RELOC, db, kf_map, cov, score, [g.frame, g.frame], [0, 1], ccap=NKF)
    where = _compare(g, recs[0], res, pm.RELOC, 0, RELOC_COL)
    _compare(g, recs[1], res, pm.RELOC, 1, RELOC_COL)
    for kf, r in where.items():
        assert int(res["score"][r:r + 1].view(np.uint32)[0]) == recs[1][1]["fields"][12 * kf + RELOC_COL], kf
    assert res["ncand"][0] == 2 and res["stats"][0, 1] > 2
