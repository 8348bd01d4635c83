"""The membership step of liborbx_placeindex.so (include/orbx_placeindex.h) in numpy: the inverted file of a sync, the count over the
postings of a query's words, the tail rows and the erase rule, giving `words` and `first` per (query, row) -- what the device hands to
the unchanged rest of the call.  tests/test_placeindex_model.py holds it to tests/place_model.py's opening().

A database is place_model's: a list of rows in add() order, (ids ascending uint32, values float64) or None for an erased row.  `drop`
names one rule to get wrong on purpose (DROPS)."""
import numpy as np

NONE = np.uint32(0xFFFFFFFF)            # `first` of a pair without a common word
DROPS = ("erased", "tail", "minimum", "query_id")


def count_of(row):
    return -1 if row is None else len(row[0])


def sync(db, n_words, rng=None):
    """The file of the rows as they stand: dict(ptr [n_words + 1], post_row, snap = the counts, count, bad = an id >= n_words).  rng: a
    permutation of the postings before they are laid out by word -- the order inside a list is the cursors', and no result may depend on it."""
    rows = np.concatenate([np.full(max(count_of(r), 0), d, np.int64) for d, r in enumerate(db)] + [np.zeros(0, np.int64)])
    words = np.concatenate([np.asarray(r[0], np.int64) for r in db if r is not None] + [np.zeros(0, np.int64)])
    bad = bool((words >= n_words).any())
    rows, words = rows[words < n_words], words[words < n_words]
    if rng is not None:
        p = rng.permutation(len(rows))
        rows, words = rows[p], words[p]
    order = np.argsort(words, kind="stable")
    ptr = np.zeros(n_words + 1, np.int64)
    np.cumsum(np.bincount(words, minlength=n_words), out=ptr[1:])
    return dict(ptr=ptr, post_row=rows[order], snap=[count_of(r) for r in db], count=len(db), bad=bad, n_words=n_words)


def stale(index, db):
    """Every query malformed: the file saw a bad id, the database lost rows, or an indexed row's count changed other than to erased."""
    if index["bad"] or len(db) < index["count"]:
        return True
    return any(count_of(db[d]) >= 0 and count_of(db[d]) != index["snap"][d] for d in range(index["count"]))


def pair_counts(index, db, q, drop=None):
    """(words [D] int32, first [D] uint32) of query q on the database as it is NOW, or None when the file is stale."""
    if stale(index, db):
        return None
    D, n_words = len(db), index["n_words"]
    live = np.array([r is not None for r in db] + [False])[:D]
    words, first = np.zeros(D, np.int32), np.full(D, NONE, np.uint32)
    ids = [int(w) for w in q[0]]
    for w in (reversed(ids) if drop == "minimum" else ids):
        if w >= n_words:
            if drop != "query_id":
                continue                                    # no postings
            w = 0
        rows = index["post_row"][index["ptr"][w]:index["ptr"][w + 1]]
        if drop != "erased":
            rows = rows[live[rows]]                         # a row erased since the sync
        np.add.at(words, rows, 1)
        if drop == "minimum":
            first[rows] = np.where(first[rows] == NONE, np.uint32(w), first[rows])      # whichever posting came first
        else:
            first[rows] = np.minimum(first[rows], np.uint32(w))
    if drop != "tail":
        qi = np.asarray(q[0], np.uint32)
        for d in range(index["count"], D):
            if db[d] is None:
                continue
            common = np.intersect1d(qi, np.asarray(db[d][0], np.uint32), assume_unique=True)
            if len(common):
                words[d], first[d] = len(common), common[0]
    return words, first


def opening(words, first, excluded=()):
    """place_model.opening()'s rows, words, max_common, min_common and scored from the pair counts (steps 1-4 without the scores)."""
    ex = set(int(e) for e in excluded)
    found = sorted((int(first[d]), d) for d in range(len(words)) if words[d] > 0 and d not in ex)
    rows = [d for _, d in found]
    w = [int(words[d]) for d in rows]
    max_common = max(w) if w else 0
    min_common = int(np.float32(max_common) * np.float32(0.8))
    return dict(rows=rows, words=w, max_common=max_common, min_common=min_common, scored=[x > min_common for x in w])
