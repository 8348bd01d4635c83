"""tests/placeindex_model.py (sync, count, tail and erase of include/orbx_placeindex.h) against tests/place_model.py's opening(): on every
planted world and every size edge of tests/place_cases.py, for every split of the rows into indexed and tail, with an erase before the
sync and one after it, under shuffled posting lists; and each of its rules is shown to matter.  CPU only."""
import numpy as np
import pytest

from tests import place_cases as pc
from tests import place_model as pm
from tests import placeindex_model as xm

WORLDS = list(pc.planted().values()) + [pc.size_edge(*s) for s in pc.SIZE_EDGES]
KEYS = ("rows", "words", "max_common", "min_common", "scored")


def n_words_of(w):
    return 1 + max([int(v[0].max()) for v in w["db"] + w["q"] if v is not None and len(v[0])] + [0])


def victim(w):
    """The row to erase: the first live row of the first query's list (a row the result depends on), else the first live row."""
    for q in w["q"]:
        rows = pm.opening(q, w["db"])["rows"]
        if rows:
            return rows[0]
    return next(d for d, r in enumerate(w["db"]) if r is not None)


def openings(index, db, w, drop=None):
    out = []
    for i, q in enumerate(w["q"]):
        c = xm.pair_counts(index, db, q, drop)
        assert c is not None
        out.append({k: v for k, v in xm.opening(*c, w["excl"][i]).items()})
    return out


def expected(db, w):
    return [{k: pm.opening(q, db, w["excl"][i])[k] for k in KEYS} for i, q in enumerate(w["q"])]


@pytest.mark.parametrize("w", WORLDS, ids=lambda w: w["name"])
def test_every_split_equals_the_dense_opening(w):
    rng = np.random.default_rng(7)
    nw, D, v = n_words_of(w), len(w["db"]), victim(w)
    erased = [None if d == v else r for d, r in enumerate(w["db"])]
    want, want_erased = expected(w["db"], w), expected(erased, w)
    assert want != want_erased or all(not o["rows"] for o in want)
    for s in range(D + 1):
        index = xm.sync(w["db"][:s], nw, rng)
        assert openings(index, w["db"], w) == want, s
        assert openings(index, erased, w) == want_erased, ("erased after the sync", s)
        assert openings(xm.sync(erased[:s], nw, rng), erased, w) == want_erased, ("erased before the sync", s)


def test_the_posting_order_changes_nothing_and_the_lists_hold_every_entry():
    w = pc.size_edge(65, 5)
    nw = n_words_of(w)
    a, b = xm.sync(w["db"], nw), xm.sync(w["db"], nw, np.random.default_rng(3))
    assert np.array_equal(a["ptr"], b["ptr"]) and not np.array_equal(a["post_row"], b["post_row"])
    assert a["ptr"][-1] == sum(len(r[0]) for r in w["db"] if r is not None) and not a["bad"]
    for word in range(nw):
        rows = sorted(b["post_row"][b["ptr"][word]:b["ptr"][word + 1]].tolist())
        assert rows == [d for d, r in enumerate(w["db"]) if r is not None and word in r[0]]
    assert openings(a, w["db"], w) == openings(b, w["db"], w)


def test_stale_files_answer_nothing():
    w = pc.size_edge(65, 5)
    nw, db = n_words_of(w), list(w["db"])
    index = xm.sync(db[:40], nw)
    assert not xm.stale(index, db) and not xm.stale(index, db[:40]) and xm.stale(index, db[:39])
    changed = list(db)
    changed[7] = (db[7][0][:-1], db[7][1][:-1])                 # another non-negative count
    assert xm.stale(index, changed) and xm.pair_counts(index, changed, w["q"][0]) is None
    back = list(db)
    assert db[4] is None
    back[4] = db[5]                                             # erased at the sync, live now
    assert xm.stale(index, back)
    gone = list(db)
    gone[7] = None
    assert not xm.stale(index, gone)
    tail_changed = list(db)
    tail_changed[50] = None
    assert not xm.stale(index, tail_changed)
    assert xm.stale(xm.sync(db, nw - 1), db) and xm.sync(db, nw - 1)["bad"]     # a database id >= n_words


def _differs(w, drop, nw=None, splits=None, erase_after=False):
    nw = nw or n_words_of(w)
    D = len(w["db"])
    v = victim(w)
    now = [None if d == v else r for d, r in enumerate(w["db"])] if erase_after else w["db"]
    for s in (splits if splits is not None else range(D + 1)):
        index = xm.sync(w["db"][:s], nw)
        assert openings(index, now, w) == expected(now, w)
        if openings(index, now, w, drop) != expected(now, w):
            return True
    return False


def test_each_rule_of_the_model_matters():
    planted = pc.planted()
    # the postings of a row erased after the sync
    assert _differs(planted["unscored_neighbour_in"], "erased", erase_after=True)
    assert not _differs(planted["unscored_neighbour_in"], "erased", erase_after=True, splits=[0])      # all tail: there are no postings
    # the tail rows
    assert _differs(planted["truncation_5_10_15"], "tail", splits=[3]) and not _differs(planted["truncation_5_10_15"], "tail", splits=[8])
    # the minimum over the postings, not whichever came first
    assert _differs(planted["equal_acc_and_first_word"], "minimum", splits=[5])
    # a query id beyond the vocabulary has no postings: here it would find word 0's
    w = pc.world("query_id_beyond", [pc.flat([0, 1, 2]), pc.flat([1, 2, 3]), pc.flat([0, 5])], [pc.flat([1, 2, 40]), pc.flat([41])])
    assert _differs(w, "query_id", nw=6, splits=[3]) and not _differs(w, "query_id", nw=42, splits=[3])
    assert set(xm.DROPS) == {"erased", "tail", "minimum", "query_id"}
