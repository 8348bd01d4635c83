"""The constructed cases of tests/kfdb_edge_cases.py are what they claim to be, by the oracle alone, and a wrong kernel could not pass them: a
plain numpy model of the query equals the oracle byte for byte on every case, and each of seven deliberately wrong variants of it differs
from the oracle on at least one.  A case that misses its edge fails here and not silently on the GPU (tests/test_gpu_kfdb_edges.py runs the
same cases).  Nothing here builds or runs a kernel."""
import functools
import os
import re

import numpy as np
import pytest

from tests import kfdb_edge_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def recorded(name):
    """The case's script as the oracle ran it: [(step, the oracle's answer)]."""
    odb, out = kc.OracleDb(), []

    def run(step):
        res = kc.apply(odb, step)
        out.append((step, res))
        return res

    kc.drive(kc.CASES[name](), run)
    return out


def _queries(name):
    return [(s, r) for s, r in recorded(name) if s[0] == "query"]


# ---- the constants --------------------------------------------------------------------------------------------------------------------
def test_the_constants_are_the_source_s():
    lines = open(os.path.join(ROOT, "orb_slam3_modified_amd", "csrc", "orbx_kfdb.hip")).read().split("\n")
    at = lambda n: lines[n - 1]   # noqa: E731
    assert int(re.search(r"constexpr int kKfdbMaxQuery = (\d+);", at(24)).group(1)) == kc.MAX_QUERY
    assert "uint32_t first = 0xffffffffu;" in at(55) and kc.NO_WORD == 0xFFFFFFFF
    assert "blockIdx.x * 4 + (threadIdx.x >> 6)" in at(53) and "blockIdx.x * 4 + (threadIdx.x >> 6)" in at(101) and kc.ROWS_PER_WG == 4
    assert "b0 += 64" in at(58) and "b0 += 64" in at(111) and kc.LANES == 64
    assert "s_qbuf + ((nq + 1) & ~1)" in at(95)
    assert "2 * db->d_rows_cap), 1024);" in at(213) and kc.ROW_TABLE == 1024
    assert "db->dead_nnz > (1u << 16) && 2 * db->dead_nnz > db->h_ids.size()" in at(279) and kc.COMPACT_DEAD == 65536
    assert "grid((nrows + 3) / 4), block(256)" in at(322) and "nq <= kKfdbMaxQuery" in at(323) and "nq <= kKfdbMaxQuery" in at(337)
    assert "(size_t)((nq + 1) & ~1) * sizeof(uint32_t) + (size_t)nq * sizeof(double)" in at(338)
    assert "lds2 > 64 * 1024 && ensure_dynamic_lds" in at(339) and kc.LDS_DEFAULT == 65536
    assert kc.score_lds_bytes(kc.LDS_LAST_DEFAULT) == 65536 == kc.LDS_DEFAULT < kc.score_lds_bytes(kc.LDS_FIRST_RAISED) == 65544
    assert kc.score_lds_bytes(kc.MAX_QUERY) == 98304 and (kc.LDS_LAST_DEFAULT, kc.LDS_FIRST_RAISED) == (5461, 5462)
    assert kc.score_lds_bytes(5463) == 12 * 5463 + 4 and kc.score_lds_bytes(5462) == 12 * 5462      # an odd count: four bytes of padding before the values


# ---- the query ladder -----------------------------------------------------------------------------------------------------------------
def test_ladder():
    p = kc.ladder_plan()
    rows, kf = p.rows, p.kf_id
    lens = sorted(len(a) for a, _ in rows.values())
    assert len(rows) == 25 and {0, 1, 63, 64, 65, 127, 128, 129, 1000, 9000, 20000} <= set(lens)
    assert len(set(kf.values())) == len(kf) and sorted(kf) == sorted(kc.LADDER_ADD_ORDER)
    added = [kf[n] for n in kc.LADDER_ADD_ORDER]
    assert added != sorted(added) and len(added) % kc.ROWS_PER_WG != 0
    every = np.concatenate([a for a, _ in rows.values()])
    assert every.min() == 0 == rows["zero"][0][0] and rows["top"][0][-1] == 0xFFFFFFFE and rows["mark"][0].tolist() == [0xFFFFFFFF]
    ordinary = every[every < 0xFFFFFFFE]
    assert ordinary.max() < kc.ID_RANGE and ordinary.max() > 1_000_000 and len(np.unique(every)) < len(every)   # some words are in several rows
    for a, v in list(rows.values()) + p.queries:
        assert a.dtype == np.uint32 and v.dtype == np.float64 and len(a) == len(v) and (np.diff(a.astype(np.int64)) > 0).all() and (v > 0).all()
    assert tuple(len(a) for a, _ in p.queries) == kc.QUERY_LENGTHS == (1, 2, 63, 64, 65, 5461, 5462, 5463, 8191, 8192, 8193, 12001)
    assert [kc.score_lds_bytes(n) > kc.LDS_DEFAULT for n in kc.QUERY_LENGTHS[5:10]] == [False, True, True, True, True]
    steps = recorded("ladder")
    asked = [len(s[1][0]) for s, _ in steps if s[0] == "query"]
    assert asked == sorted(asked) and asked[::2] == list(kc.QUERY_LENGTHS)                 # ascending, each with and without the exclusions
    assert [len(s[1]) for s, _ in steps if s[0] == "sharing"] == list(kc.QUERY_LENGTHS)
    assert len(p.exclude) == 3 and set(p.exclude) <= set(kf.values())

    common = lambda q, n: np.flatnonzero(np.isin(rows[n][0], q[0]))   # noqa: E731   positions of the row's words the query holds
    by_len = {len(q[0]): q for q in p.queries}
    res = {len(s[1][0]): r for s, r in steps if s[0] == "query" and not s[2]}
    words_of = lambda L, n: dict(zip(res[L]["kf"].tolist(), res[L]["words"].tolist())).get(kf[n], 0)   # noqa: E731
    # the 1-word query: the last word of the 20 000-word row and nothing else
    assert common(by_len[1], "huge").tolist() == [19999] and res[1]["kf"].tolist() == [kf["huge"]] and res[1]["words"].tolist() == [1]
    assert res[1]["max_common"] == 1 and res[1]["min_common"] == 0 and 0 < res[1]["score"][0] < 1
    assert sorted(res[2]["kf"].tolist()) == sorted([kf["zero"], kf["top"]]) and res[2]["kf"][0] == kf["zero"]
    for L in kc.QUERY_LENGTHS[2:]:
        q = by_len[L]
        assert q[0][0] == 0 and q[0][-1] == (0xFFFFFFFF if L in kc.MARK_QUERIES else 0xFFFFFFFE)       # the query's first and last word are in a row
        assert (19999 not in common(q, "huge")) and len(common(q, "huge")) >= 1
        c = common(q, "late")
        assert len(c) >= 2 and c.min() == 64 and c.max() == 128 and words_of(L, "late") == len(c)      # nothing in its first trip
        assert common(q, "only63").tolist() == [63] and words_of(L, "only63") == 1                     # the last lane of a trip, the row's last word
        assert common(q, "only64").tolist() == [64] and words_of(L, "only64") == 1                     # the first lane of the second trip
        c = common(q, "ends")
        assert c[0] == 0 and c[-1] == 999                                                              # a row's first and last word
        assert common(q, "zero")[0] == 0 and common(q, "top")[-1] == 64
        assert (words_of(L, "mark") == 1) == (L in kc.MARK_QUERIES)
        hit = {n for n in rows if len(common(q, n))}
        assert hit >= set(rows) - {"empty", "mark"}                                                    # every row that has a word
        assert len(res[L]["kf"]) == len(hit) and (res[L]["score"] >= 0).sum() >= 1
    assert words_of(12001, "huge") > 3000 and words_of(8192, "big") > 1000                            # thousands of common words
    ex = {len(s[1][0]): r for s, r in steps if s[0] == "query" and s[2]}
    assert all(not set(p.exclude) & set(ex[L]["kf"].tolist()) for L in kc.QUERY_LENGTHS)
    assert 1000 < ex[12001]["max_common"] < res[12001]["max_common"] and ex[8192]["kf"].size == res[8192]["kf"].size - 3
    assert ex[1]["kf"].size == 0 and ex[1]["max_common"] == 0                                          # the 1-word query's only keyframe excluded
    for s, r in steps:
        if s[0] == "score":                                                                            # every row against every query
            assert len(r) == len(rows) and (r[[len(rows[n][0]) == 0 for n in kc.LADDER_ROWS]].tobytes() == np.float64(-0.0).tobytes())
            assert len(s[1][0]) < 63 or (r > 0).sum() >= 22
    print("ladder:", {L: (len(res[L]["kf"]), res[L]["max_common"], int((res[L]["score"] >= 0).sum())) for L in kc.QUERY_LENGTHS})


# ---- the row-count ladder -------------------------------------------------------------------------------------------------------------
def test_row_counts():
    p = kc.rows_plan()
    steps = [s for s, _ in recorded("rows")]
    sizes, n = [], 0
    for s in steps:                                # the number of rows in the table at every query
        n = 0 if s[0] == "clear" else n + (s[0] == "add")
        if s[0] == "query":
            sizes.append(n)
    assert sizes[:10] == [1, 1, 2, 2, 3, 3, 4, 4, 5, 5] and sizes[10:14] == [1023, 1024, 1025, 1025] and sizes[14:] == [1125, 1125]
    assert all(8 <= len(a) <= 16 for a, _ in p.grown) and len(p.pool) == kc.ROWS_POOL and len(set(p.ids)) == kc.ROW_TABLE + 1
    assert kc.host_compactions(steps) == []        # the erased rows stay in the table: the re-added ones lie past row 1024
    assert len(p.erased) == 300 and len(p.readded) == 100 and set(p.readded) <= set(p.erased)
    row_of = {}
    n = 0
    for s in steps[steps.index(("clear",), 40):]:  # the last database: row index of every alive keyframe
        if s[0] == "clear":
            n, row_of = 0, {}
        elif s[0] == "add":
            row_of[s[1]] = n
            n += 1
        elif s[0] == "erase":
            row_of.pop(s[1], None)
    sel = [row_of[k] for k in p.selection]
    assert min(sel) < 100 and sum(r < 1024 for r in sel) >= 30 and sum(r > 1024 for r in sel) >= 30 and len(row_of) == 825
    q = [(s, r) for s, r in recorded("rows") if s[0] == "query"]
    listed = [len(r["kf"]) for _, r in q]
    assert [a <= b for a, b in zip(listed, sizes)] == [True] * len(q) and max(listed[:10]) >= 4 and min(listed[0:10:2]) >= 1
    assert min(listed[10:13]) > 900 and listed[13] < listed[10] and min(listed[14:]) > 700                # nearly every row shares a word
    kf, words = [r for s, r in recorded("rows") if s[0] == "sharing"][-1]
    assert len(kf) > 700 and {row_of[int(k)] > 1024 for k in kf} == {True, False}
    first = np.array([min(set(p.bow_of[int(k)][0].tolist()) & set(p.queries[5][0].tolist())) for k in kf])
    assert (np.diff(first.astype(np.int64)) >= 0).all() and len(np.unique(first)) < len(first) // 4      # long runs of ties in the list


# ---- the compaction step --------------------------------------------------------------------------------------------------------------
def test_compaction():
    p = kc.compaction_plan()
    assert len(p.rows) == kc.COMPACT_KFS == 40 and all(1900 <= len(a) <= 2100 for a, _ in p.rows)
    nnz = sum(p.lengths)
    dead = np.cumsum(p.lengths)
    rule = (dead > kc.COMPACT_DEAD) & (2 * dead > nnz)
    assert p.at is not None and 0 < p.at < kc.COMPACT_KFS - 4 and not rule[:p.at].any() and rule[p.at]   # false before the named erase, true at it
    assert dead[p.at - 1] <= kc.COMPACT_DEAD < dead[p.at]                                                # ... by the 65 536 entries, not by the half
    steps = [s for s, _ in recorded("compaction")]
    at = kc.host_compactions(steps)
    assert len(at) == 1 and steps[at[0]] == ("erase", p.ids[p.order[p.at]])
    assert steps[at[0] - 1][0] == "sharing" and steps[at[0] - 2][0] == "query" and steps[at[0] + 1][0] == "query"
    assert steps[at[0] - 2][1] is steps[at[0] + 1][1]                                                    # the same query on both sides of the step
    before, after = recorded("compaction")[at[0] - 2][1], recorded("compaction")[at[0] + 1][1]
    assert len(before["kf"]) == len(after["kf"]) + 1 == kc.COMPACT_KFS - p.at and (after["score"] >= 0).any()
    last = _queries("compaction")[-1][1]
    assert len(last["kf"]) == kc.COMPACT_KFS - p.at - 1 + 5 and last["kf"][-1] != p.new[1][0]
    assert {900001, 7} <= set(last["kf"].tolist()) and {p.ids[i] for i in p.order[:3]} <= set(last["kf"].tolist())


# ---- list order -----------------------------------------------------------------------------------------------------------------------
def test_list_order():
    p = kc.order_plan()
    steps = [s for s, _ in recorded("order")]
    assert kc.ORDER_GROUPS >= 3 and kc.ORDER_MEMBERS >= 4
    qset = set(p.query[0].tolist())
    for g, (ids, _) in p.members:
        assert min(set(ids.tolist()) & qset) == p.qw[3 + 9 * g]                                         # the group's one first shared word
    assert len(set(p.ids)) == len(p.ids) and sorted(p.ids) != p.ids and max(np.diff(sorted(p.ids))) > 100
    added = [s[1] for s in steps if s[0] == "add"][:12]
    assert added != sorted(added) and added != sorted(added, reverse=True)
    at = kc.host_compactions(steps)
    assert len(at) == 1 and steps[at[0]] == ("erase", p.fillers[-1][0])                                 # one pass through the compaction
    group_of = {k: g for k, (g, _) in zip(p.ids, p.members)}
    lists = []
    for s, r in _queries("order"):
        kf = [int(k) for k in r["kf"] if int(k) in group_of]
        gs = [group_of[k] for k in kf]
        assert gs == sorted(gs)                                                                        # groups in the order of their words ...
        lists.append(kf)
    assert len(lists) == 5 and len(lists[0]) == len(lists[2]) == len(lists[3]) == 24 and len(lists[1]) == 24 - len(p.back1) and len(lists[4]) == 23
    assert lists[0] != lists[2] and sorted(lists[0]) == sorted(lists[2]) and lists[2] == lists[3]
    for g in range(kc.ORDER_GROUPS):                                                                   # ... and inside a group the order of the adds
        back = [p.ids[j] for j in reversed(p.back1) if p.members[j][0] == g]
        mine = [k for k in lists[2] if group_of[k] == g]
        assert len(back) >= 1 and mine[-len(back):] == back
        assert mine != sorted(mine) and [k for k in lists[0] if group_of[k] == g] != sorted(mine)
    n_fill = [sum(int(k) >= 700000 for k in r["kf"]) for _, r in _queries("order")]
    assert n_fill == [8, 8, 8, 0, 0]


# ---- thresholds -----------------------------------------------------------------------------------------------------------------------
def test_thresholds():
    p = kc.thresholds_plan()
    qset = set(p.query[0].tolist())
    assert len(qset) == 12 and [c for _, c, _ in p.kfs] == [c for c in range(13) for _ in range(2)]
    assert all(len(set(b[0].tolist()) & qset) == c for _, c, b in p.kfs)
    q = _queries("thresholds")
    known = {k for k, _, _ in p.kfs}
    walk = [(r["max_common"], r["min_common"]) for s, r in q[0:4 * 13:4]]
    assert walk == [(m, int(np.float32(m) * np.float32(0.8))) for m in (12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1)] + [(0, 0)]
    assert [mn for _, mn in walk] == [9, 8, 8, 7, 6, 5, 4, 4, 3, 2, 1, 0, 0]
    for i in range(13):
        (s0, r0), floors = q[4 * i], [s[3] for s, _ in q[4 * i:4 * i + 4]]
        mx, mn = r0["max_common"], r0["min_common"]
        assert floors == [0, mn, mx, mx + 1] and all(s[2] == s0[2] for s, _ in q[4 * i:4 * i + 4])
        assert len(r0["kf"]) == 2 * mx and sorted(r0["words"].tolist()) == [c for c in range(1, mx + 1) for _ in range(2)]
        assert int((r0["score"] >= 0).sum()) == 2 * (mx - mn)
        r1, r2, r3 = (r for _, r in q[4 * i + 1:4 * i + 4])
        assert r1["score"].tobytes() == r0["score"].tobytes() and (r2["score"] == -1).all() and (r3["score"] == -1).all()
        assert (r2["min_common"], r3["min_common"]) == ((mx, mx + 1) if mx else (0, 0)) and r2["max_common"] == r3["max_common"] == mx
        ex = s0[2]
        if i:
            assert len(set(ex) & known) == 2 * i and set(ex) - known and len(ex) > len(set(ex))        # unknown ids and repeated ones
    assert len(q) == 4 * 13 + 4
    for s, r in q[-4:]:                                                                                # everything excluded
        assert known <= set(s[2]) and r["kf"].size == 0 and r["max_common"] == 0 and r["min_common"] == 0
    assert [s[3] for s, _ in q[-4:]] == [0, 0, 0, 1]


# ---- score arithmetic -----------------------------------------------------------------------------------------------------------------
def test_score_inputs():
    p = kc.score_plan()
    for qi, q in enumerate(p.queries):
        for b in p.rows:
            pos = np.flatnonzero(np.isin(b[0], q[0]))
            assert len(b[0]) >= 300 and len(pos) >= 200 and len(np.unique(pos // kc.LANES)) >= 5       # over several trips of the wave
    every = np.concatenate([v for _, v in p.rows + p.queries])
    pos = every[every > 0]
    assert (every == 0).sum() > 50 and pos.min() < 1e-8 and pos.max() > 0.1 and (every >= 0).all()
    assert np.array_equal(p.queries[-1][0], p.rows[4][0]) and p.queries[-1][1].tobytes() == p.rows[4][1].tobytes()
    assert all(len(np.intersect1d(p.apart[0], b[0])) == 0 for b in p.rows + p.queries)
    sc = [(s, r) for s, r in recorded("score") if s[0] == "score"]
    assert [len(s[2]) for s, _ in sc[:kc.SCORE_QUERIES]] == [kc.SCORE_ROWS] * kc.SCORE_QUERIES
    main = np.array([r for _, r in sc[:kc.SCORE_QUERIES]])
    assert (main > 0).all() and len(np.unique(main)) == main.size
    s, r = sc[kc.SCORE_QUERIES]                                                                        # the same keyframe three times, one apart
    assert s[2].count(p.ids[3]) == 3 and r[0].tobytes() == r[1].tobytes() == r[4].tobytes() and r[0] > 0
    assert r[2].tobytes() == np.float64(-0.0).tobytes() and s[2][2] == p.apart_id                      # no common word: -0.0
    assert sc[kc.SCORE_QUERIES + 1][1][1].tobytes() == np.float64(-0.0).tobytes()
    s, r = sc[kc.SCORE_QUERIES + 2]                                                                    # the empty query: -0.0 too
    assert len(s[1][0]) == 0 and r.tobytes() == np.array([-0.0, -0.0]).tobytes()
    s, r = sc[kc.SCORE_QUERIES + 3]                                                                    # weight 0 throughout
    assert (s[1][1] == 0).all() and r.tobytes() == np.full(4, -0.0).tobytes()
    q = _queries("score")
    assert q[-2][1]["score"].tobytes().count(np.float64(-0.0).tobytes()) >= 2 and (q[-2][1]["score"] != -1).sum() >= 2   # -0.0 through query
    assert q[-1][1]["kf"].size == 0 and len(q[-1][0][1][0]) == 0
    for s, r in q:
        if s[3] == 100:                                                                                # a floor among the counts
            assert r["min_common"] == max(100, int(np.float32(r["max_common"]) * np.float32(0.8))) and r["words"].min() < r["max_common"]


# ---- the model and its wrong variants -------------------------------------------------------------------------------------------------
class Model:
    """The query as the kernels compute it, in numpy: per row the words found in the query by search, the list sorted by (first shared word,
    order of the adds), minCommonWords = (int)(maxCommonWords * 0.8f) raised to the floor, a score where words > minCommonWords, the terms
    added serially in ascending word order.  `wrong` names one deliberate error."""
    WRONG = ("ties_by_id", "greater_equal", "miss_query_last", "miss_row_first", "descending", "lane_partials", "plus_zero")

    def __init__(self, wrong=None):
        assert wrong is None or wrong in self.WRONG
        self.wrong, self.seq = wrong, 0
        self.clear()

    def clear(self):
        self.rows = {}

    def __len__(self):
        return len(self.rows)

    def add(self, kf_id, bow):
        self.rows[kf_id] = (bow[0].astype(np.int64), bow[1], self.seq)
        self.seq += 1

    def erase(self, kf_id):
        self.rows.pop(kf_id, None)

    def _common(self, q, ids):
        """Positions in the row and in the query of the words they share."""
        if self.wrong == "miss_query_last":
            q = q[:-1]
        if len(q) == 0 or len(ids) == 0:
            return np.zeros(0, np.int64), np.zeros(0, np.int64)
        pos = np.searchsorted(q, ids)
        hit = q[np.minimum(pos, len(q) - 1)] == ids
        if self.wrong == "miss_row_first":
            hit[0] = False
        return np.flatnonzero(hit), pos[hit]

    def _score(self, qv, vals, rj, qj):
        vi, wi = qv[qj], vals[rj]
        t = np.abs(vi - wi) - np.abs(vi) - np.abs(wi)
        serial = lambda x: float(np.add.accumulate(x)[-1]) if len(x) else 0.0   # noqa: E731   one rounding a term, in order
        if self.wrong == "descending":
            s = serial(t[::-1])
        elif self.wrong == "lane_partials":
            s = serial(np.array([serial(t[rj % kc.LANES == lane]) for lane in range(kc.LANES)]))
        else:
            s = serial(t)
        s = -s / 2.0
        return s + 0.0 if self.wrong == "plus_zero" else s

    def query(self, bow, exclude=(), min_words_floor=0):
        q, qv = bow[0].astype(np.int64), bow[1]
        ex = set(exclude)
        found = []
        for k, (ids, vals, seq) in self.rows.items():
            if k in ex:
                continue
            rj, qj = self._common(q, ids)
            if len(rj):
                found.append((int(ids[rj[0]]), k if self.wrong == "ties_by_id" else seq, k, rj, qj))
        found.sort(key=lambda f: f[:2])
        kf = np.array([f[2] for f in found], np.int64)
        words = np.array([len(f[3]) for f in found], np.int32)
        if not found:
            return dict(kf=kf, words=words, score=np.zeros(0), max_common=0, min_common=0)
        mx = int(words.max())
        mn = max(int(np.float32(mx) * np.float32(0.8)), min_words_floor)
        score = np.full(len(found), -1.0)
        for i, f in enumerate(found):
            if words[i] >= mn if self.wrong == "greater_equal" else words[i] > mn:
                score[i] = self._score(qv, self.rows[f[2]][1], f[3], f[4])
        return dict(kf=kf, words=words, score=score, max_common=mx, min_common=mn)

    def sharing(self, word_ids):
        r = self.query((np.asarray(word_ids, np.uint32), np.ones(len(word_ids))), [], 2 ** 30)    # nothing is scored
        return r["kf"], r["words"]

    def score(self, bow, kf_ids):
        q, qv = bow[0].astype(np.int64), bow[1]
        return np.array([self._score(qv, self.rows[k][1], *self._common(q, self.rows[k][0])) for k in kf_ids], np.float64)


def _differences(name, wrong):
    """The steps of the case on which the model's answer is not the oracle's, byte for byte; and for the first block of score steps of the
    score case the number of (query, keyframe) pairs that differ and their total."""
    m = Model(wrong)
    bad, pairs, npairs, nscore = [], 0, 0, 0
    for i, (step, want) in enumerate(recorded(name)):
        got = kc.apply(m, step)
        if step[0] == "query":
            same = np.array_equal(got["kf"], want["kf"]) and np.array_equal(got["words"], want["words"]) and \
                (got["max_common"], got["min_common"]) == (want["max_common"], want["min_common"]) and got["score"].tobytes() == want["score"].tobytes()
        elif step[0] == "sharing":
            same = np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        elif step[0] == "score":
            same = got.tobytes() == want.tobytes()
            if name == "score" and nscore < kc.SCORE_QUERIES:
                pairs += int((got.view(np.uint64) != want.view(np.uint64)).sum())
                npairs += len(want)
            nscore += 1
        else:
            same = True
        if not same:
            bad.append(i)
    return bad, pairs, npairs


@pytest.mark.parametrize("name", sorted(kc.CASES))
def test_model_equals_oracle(name):
    bad, _, _ = _differences(name, None)
    assert bad == [], (name, bad[:5], [recorded(name)[i][0][0] for i in bad[:5]])
    assert sum(s[0] in ("query", "sharing", "score") for s, _ in recorded(name)) >= 7


# the cases on which each wrong variant has to show, and may show nowhere else without being looked at
RAILS = dict(ties_by_id=("order", "rows"), greater_equal=("thresholds",), miss_query_last=("ladder",), miss_row_first=("ladder",),
             descending=("score",), lane_partials=("score",), plus_zero=("score",))


@pytest.mark.parametrize("wrong", Model.WRONG)
def test_wrong_model_differs_from_oracle(wrong):
    assert set(RAILS) == set(Model.WRONG)
    for name in RAILS[wrong]:
        bad, pairs, npairs = _differences(name, wrong)
        print(f"{wrong} on {name}: {len(bad)} of {len(recorded(name))} steps differ" + (f", {pairs} of {npairs} scored pairs" if npairs else ""))
        assert bad, (wrong, name)
        if wrong in ("descending", "lane_partials"):
            assert npairs == kc.SCORE_QUERIES * kc.SCORE_ROWS == 50 and 2 * pairs >= npairs, (wrong, pairs, npairs)
    if wrong == "plus_zero":                       # through score and through query
        bad, _, _ = _differences("score", wrong)
        ops = {recorded("score")[i][0][0] for i in bad}
        assert ops == {"score", "query"}
