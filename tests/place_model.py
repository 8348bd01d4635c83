"""The specification of the batched place recognition (include/orbx_place.h) in numpy: steps 1-7 of
KeyFrameDatabase::DetectRelocalizationCandidates and DetectNBestCandidates (src/KeyFrameDatabase.cc:733-845, :604-730), float32 and double
where the reference has them, one query after the other on one score array.  tests/test_place_model.py holds this file to the oracle's
mo_kfdb_query (steps 1-4) and to the reference's recorded results (the whole routine); liborbx_place.so is held to this file.

A database is a list of rows in add() order, each (ids ascending uint32, values float64) or None for an erased row.  `drop` names one
rule to get wrong on purpose (DROPS): the tests use it to show that a constructed case depends on its rule."""
import numpy as np

from tests import score_model as sm

RELOC, NBEST = 0, 1
COV = 10
F32 = np.float32
DROPS = ("unscored_neighbour", "earlier_query", "stable_sort", "tie_by_row", "first_word", "truncation", "dedup", "map", "self_neighbour",
         "exclusion", "strict_threshold", "full_count")


def opening(q, db, excluded=(), drop=None, marked=()):
    """Steps 1-4 for one query: dict(rows = the rows in the query in list order, words = their common-word counts, max_common, min_common,
    scored = bool per list entry, si = float32 per list entry (only where scored)).  marked: rows that already carry this query's id in
    their mn*Query field because the same id asked before (:623, :748): the reference does not list them again.  The library's contract
    is ids that never repeat; only the comparison with the reference's recorded results passes a mark."""
    ex = set() if drop == "exclusion" else set(int(e) for e in excluded)
    ex |= set(int(m) for m in marked)
    qi = np.asarray(q[0], np.uint32)
    found = []
    for d, row in enumerate(db):
        if row is None or d in ex:
            continue
        common = np.intersect1d(qi, np.asarray(row[0], np.uint32), assume_unique=True)
        if len(common):
            found.append((0 if drop == "first_word" else int(common[0]), -d if drop == "tie_by_row" else d, d, len(common)))
    found.sort()
    rows = [f[2] for f in found]
    words = [f[3] for f in found]
    max_common = max(words) if words else 0
    factor = np.nextafter(F32(0.8), F32(0.0)) if drop == "truncation" else F32(0.8)      # 0.79999995: one word less at 5, 10 and 15
    min_common = int(F32(max_common) * factor)
    scored = [w >= min_common if drop == "strict_threshold" else w > min_common for w in words]
    si = [F32(sm.score_fast(sm.L1_NORM, q, db[d])) if s else None for d, s in zip(rows, scored)]
    return dict(rows=rows, words=words, max_common=max_common, min_common=min_common, scored=scored, si=si)


def tail(kind, op, kf_score, entry_score, kf_map, kf_cov, q_map, n_candidates, drop=None, bad_maps=(), marked=()):
    """Steps 4 (the score field) to 7 for one query on the opening `op`; kf_score (float32 [D]) is updated.  entry_score: the array as the
    CALL found it (what drop = "earlier_query" reads instead).  bad_maps: map ids whose IsBad() is true -- the reference's merge test
    (:721), which the library leaves to its caller (no keyframe of a bad map in the database); only the comparison with the reference's
    recorded results passes it.  marked: as in opening(); a marked row passes the neighbour test (:686, :807), erased or not.
    -> (cand, merge) as lists of rows."""
    member = set(op["rows"]) | set(int(m) for m in marked)
    lst = [(d, s) for d, s, on in zip(op["rows"], op["si"], op["scored"]) if on]
    mine = {d for d, _ in lst}
    for d, s in lst:
        kf_score[d] = s
    acc_holder = []
    for d, s in lst:
        acc, best, holder = F32(s), F32(s), d
        for c in kf_cov[d]:
            c = int(c)
            if c < 0 or c not in member:
                continue
            if drop == "self_neighbour" and c == d:
                continue
            if c not in mine:
                if drop == "unscored_neighbour":
                    continue
                s2 = F32(entry_score[c]) if drop == "earlier_query" else F32(kf_score[c])
            else:
                s2 = F32(kf_score[c])
            acc = F32(acc + s2)
            if s2 > best:
                holder, best = c, s2
        acc_holder.append((acc, holder))
    same = lambda h: drop == "map" or int(kf_map[h]) == int(q_map)   # noqa: E731
    if kind == RELOC:
        best_acc = F32(0.0)
        for a, _ in acc_holder:
            if a > best_acc:
                best_acc = a
        min_retain = F32(F32(0.75) * best_acc)
        cand, seen = [], set()
        for a, h in acc_holder:
            if a > min_retain:
                if not same(h):
                    continue
                if drop == "dedup" or h not in seen:
                    cand.append(h)
                    seen.add(h)
        return cand, []
    order = sorted(range(len(acc_holder)), key=lambda i: (-float(acc_holder[i][0]), -i if drop == "stable_sort" else i))
    loop, merge, seen = [], [], set()
    for i in order:
        if len(loop) >= n_candidates and len(merge) >= n_candidates:
            break
        h = acc_holder[i][1]
        if drop == "dedup" or h not in seen:
            if same(h) and len(loop) < n_candidates:
                loop.append(h)
            elif not same(h) and len(merge) < n_candidates and int(kf_map[h]) not in bad_maps:
                merge.append(h)
            seen.add(h)
    return loop, merge


def run(kind, db, kf_map, kf_cov, kf_score, queries, q_map, excl=None, n_candidates=0, ccap=8, drop=None, openings=None, bad_maps=(), marked=None):
    """The call: queries in order on one score array.  -> dict(cand [Q, ccap], ncand [Q], merge, nmerge (N-best, else None), stats [Q, 4],
    score = the OUT array float32 [D]).  `openings`: step 1-4 results computed elsewhere (per query), used instead of opening()."""
    nq = len(queries)
    score = np.array(kf_score, np.float32)
    entry = score.copy()
    cand, merge = np.full((nq, ccap), -1, np.int32), np.full((nq, ccap), -1, np.int32)
    ncand, nmerge, stats = np.zeros(nq, np.int32), np.zeros(nq, np.int32), np.zeros((nq, 4), np.int32)
    for i, q in enumerate(queries):
        ex = excl[i] if (kind == NBEST and excl is not None) else ()
        mk = marked[i] if marked is not None else ()
        op = openings[i] if openings is not None else opening(q, db, ex, drop, mk)
        c, m = tail(kind, op, score, entry, kf_map, kf_cov, q_map[i], n_candidates, drop, bad_maps, mk)
        stats[i] = (len(op["rows"]), sum(op["scored"]), op["max_common"], op["min_common"])
        ncand[i], nmerge[i] = (min(len(c), ccap), min(len(m), ccap)) if drop == "full_count" else (len(c), len(m))
        cand[i, :min(len(c), ccap)] = c[:ccap]
        merge[i, :min(len(m), ccap)] = m[:ccap]
    two = kind == NBEST
    return dict(cand=cand, ncand=ncand, merge=merge if two else None, nmerge=nmerge if two else None, stats=stats, score=score)
