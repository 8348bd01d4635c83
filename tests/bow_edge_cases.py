"""Constructed inputs at the size edges of the batched bag of words (liborbx_bow.so), stated once: the GPU suite runs them
(tests/test_gpu_bow_batch_edges.py) and the CPU suite checks with the oracle alone that each case is what it claims to be
(tests/test_bow_edge_cases.py).  Descriptor rows are chosen by the oracle's descent, BowVectors for the score matrix are written down directly.
Everything is deterministic (fixed seeds) and nothing here needs a GPU."""
import math
from collections import namedtuple

import numpy as np

from oracle import pyoracle as po
from tests.vocab_util import make_vocabulary

KEY_LDS = 4096       # kBowLds, orb_slam3_modified_amd/csrc/bow/orbx_bow.hip:32: a frame of at most this many features sorts its keys in LDS
QUERY_LDS = 4000     # kScoreLds, orb_slam3_modified_amd/csrc/bow/orbx_bow.hip:33: a query of at most this many entries is staged in LDS
LDS_LIMITS = (None, 0, KEY_LDS - 1, KEY_LDS, KEY_LDS + 1)   # ORBX_BOW_LDS at orbx_bow_create (None: unset; include/orbx_bow.h:19 clamps to 0 .. 4096)

CAP = 4229           # descriptor rows a frame: past both limits, no multiple of 4 or 64
POOL = 6000          # random descriptors the trees are built on and the frames draw from
POOL_SEED = 20261

# name -> k, L, levelsup of the FeatureVector, and how the words get their weights:
#   "idf"   DBoW2's IDF rule, log(N / Ni), over DOCS documents (setNodeWeights, TemplatedVocabulary.h:803-861): a word every document holds
#           weighs exactly 0, a word no document holds keeps the 0 it started with
#   "drawn" vocab_util's own: U(0.5, 8), and 0 for a fraction of the words
TREES = {"idf": dict(k=6, L=3, levelsup=1, weights="idf", seed=63), "drawn": dict(k=9, L=2, levelsup=0, weights="drawn", seed=92)}
DOCS = 40
STOP_WORDS = 5       # the most frequent words of the pool are put into every document
DRAWN_ZERO_FRAC = 0.1


def pool():
    return np.random.default_rng(POOL_SEED).integers(0, 256, (POOL, 32), dtype=np.uint8)


def _set_header(path, k, L, scoring, weighting):
    lines = open(path).read().split("\n")
    lines[0] = f"{k} {L} {scoring} {weighting}"
    open(path, "w").write("\n".join(lines))


def vocabulary_file(path, tree, scoring=0, weighting=0):
    """The text file of TREES[tree] with the given header.  The tree and its weights do not depend on the header, as in a file DBoW2 saved and
    somebody edited: the weights are what the file says."""
    t = TREES[tree]
    k, L = t["k"], t["L"]
    d = pool()
    make_vocabulary(path, d, k, L, seed=t["seed"], zero_weight_frac=DRAWN_ZERO_FRAC if t["weights"] == "drawn" else 0.0)
    if t["weights"] == "idf":
        word = po.OracleVocabulary(path).descend(d, 0)[0]
        nwords = int(word.max()) + 1
        stop = np.argsort(-np.bincount(word, minlength=nwords), kind="stable")[:STOP_WORDS]
        per = POOL // DOCS
        ni = np.zeros(nwords, np.int64)
        for i in range(DOCS):       # document i: the pool's rows [i * per, (i + 1) * per) and one row of every stop word
            ni[np.union1d(word[i * per:(i + 1) * per], stop)] += 1
        lines = open(path).read().split("\n")
        w = 0
        for j in range(1, len(lines)):
            tok = lines[j].split(" ")
            if int(tok[1]) > 0:
                tok[-1] = repr(math.log(DOCS / ni[w]) if ni[w] > 0 else 0.0)
                w += 1
            lines[j] = " ".join(tok)
        open(path, "w").write("\n".join(lines))
    _set_header(path, k, L, scoring, weighting)
    return path


def leaf_descriptors(path):
    """The words' own descriptors, in word order."""
    rows = [ln.split(" ") for ln in open(path).read().split("\n")[1:] if ln.strip()]
    return np.array([[int(b) for b in r[2:34]] for r in rows if int(r[1]) > 0], np.uint8)


# ---- transform ------------------------------------------------------------------------------------------------------------------------
# One frame of the batch.  rows: the frame's descriptors (its count is len(rows)); None: the count is -1.  kept: the number of features whose
# word weighs more than 0, which is the number of keys the kernel sorts.  zero: positions of the weight-0 features the case is about.
Frame = namedtuple("Frame", "name rows kept zero")

KEPT_COUNTS = (0, 1, 2, 3, 63, 64, 65, 511, 512, 513, KEY_LDS - 1, KEY_LDS, KEY_LDS + 1, CAP)


def transform_frames(path):
    """The batch for the vocabulary file `path` (any header), as a list of Frames."""
    ov = po.OracleVocabulary(path)
    d = np.concatenate([pool(), leaf_descriptors(path)])
    word, weight, _ = ov.descend(d, 0)
    keep, drop = np.flatnonzero(weight > 0), np.flatnonzero(~(weight > 0))
    rng = np.random.default_rng(POOL_SEED + 1)
    frames = {}

    def mixed(name, nkeep, ndrop):
        """nkeep kept and ndrop weight-0 features, shuffled."""
        idx = np.concatenate([rng.choice(keep, nkeep), rng.choice(drop, ndrop)])
        frames[name] = Frame(name, d[rng.permutation(idx)], nkeep, None)

    for n in KEPT_COUNTS:           # the small frames carry some weight-0 features too, the large ones have count == kept
        mixed(f"kept{n}", n, 0 if n == 0 or n >= KEY_LDS - 1 else n % 5 + 1)
    hits = np.bincount(word[keep])
    one = int(np.argmax(hits))      # the kept word most of the pool falls into
    for n in (KEY_LDS, KEY_LDS + 1):
        frames[f"oneword{n}"] = Frame(f"oneword{n}", d[rng.choice(np.flatnonzero(word == one), n)], n, None)
    every = rng.permutation(np.unique(word, return_index=True)[1])    # one row for every word, the words in a shuffled order
    frames["everyword"] = Frame("everyword", d[every], int((weight[every] > 0).sum()), None)
    frames["allzero"] = Frame("allzero", d[rng.choice(drop, 300)], 0, np.arange(300))
    idx = rng.choice(drop, 300)
    idx[170] = keep[11]
    frames["allbutone"] = Frame("allbutone", d[idx], 1, np.delete(np.arange(300), 170))
    idx = np.concatenate([rng.choice(drop, 64), rng.choice(keep, KEY_LDS)])          # more features than the LDS holds, exactly as many keys
    frames["zerofirst64"] = Frame("zerofirst64", d[idx], KEY_LDS, np.arange(64))
    idx = np.concatenate([rng.choice(keep, 960), rng.choice(drop, 64)])              # rows 960 .. 1023: one whole wave of the second pass
    frames["zerolast64"] = Frame("zerolast64", d[idx], 960, np.arange(960, 1024))
    frames["overflow"] = Frame("overflow", None, 0, None)
    order = [f"kept{n}" for n in KEPT_COUNTS[:10]] + ["everyword", "allzero", "allbutone", "zerolast64", f"kept{KEY_LDS - 1}", f"kept{KEY_LDS}",
             f"oneword{KEY_LDS}", f"oneword{KEY_LDS + 1}", "zerofirst64", f"kept{KEY_LDS + 1}", "overflow", f"kept{CAP}"]
    assert sorted(order) == sorted(frames)
    return [frames[n] for n in order]


def transform_batch(frames, variant):
    """desc [B, CAP, 32] uint8 and counts [B, 2] int32 (the second column is what a batch extraction leaves there: not read).  The rows past
    each count hold 0xFF in every other frame and random bytes in the rest; `variant` (0 or 1) says which frames get which."""
    rng = np.random.default_rng(POOL_SEED + 2 + variant)
    B = len(frames)
    desc = rng.integers(0, 256, (B, CAP, 32), dtype=np.uint8)
    counts = np.zeros((B, 2), np.int32)
    for f, fr in enumerate(frames):
        n = -1 if fr.rows is None else len(fr.rows)
        counts[f] = (n, 12345 + f)
        if (f + variant) % 2 == 0:
            desc[f] = 0xFF
        if n > 0:
            desc[f, :n] = fr.rows
    return desc, counts


# ---- score matrix ---------------------------------------------------------------------------------------------------------------------
Q_CAP, DB_CAP = 8192, 8200     # the strides of the two sides; the longest query fills its stride
NQ, NDB = 7, 513
SHAPES = [(nq, ndb) for nq in (1, NQ) for ndb in (1, 255, 256, 257, NDB)]
ID_RANGE = 40000               # ordinary ids are drawn below this
TOP_ID = 0xFFFFFFFF            # the largest id a uint32 entry holds
QUERY_LENGTHS = (0, 1, QUERY_LDS - 1, QUERY_LDS, QUERY_LDS + 1, Q_CAP, -1)   # -1: the overflow marker, scored as an empty vector

ScoreCases = namedtuple("ScoreCases", "q db patterns")   # q, db: lists of (ids uint32 ascending, values float64); patterns: name -> [(qi, di)]


def _normalised(rng, ids):
    """Positive values for `ids`, divided by their running sum in ascending id order (BowVector::normalize, BowVector.cpp:61-85)."""
    ids = np.asarray(ids, np.uint32)
    assert len(ids) == 0 or (np.diff(ids.astype(np.int64)) > 0).all()
    v = rng.uniform(0.05, 1.0, len(ids))
    return ids, (v / np.cumsum(v)[-1] if len(ids) else v)


def _draw(rng, n, lo=0, hi=ID_RANGE, avoid=()):
    """n sorted distinct ids in [lo, hi) that are not in `avoid`."""
    free = np.setdiff1d(np.arange(lo, hi, dtype=np.int64), np.asarray(avoid, np.int64))
    return np.sort(rng.choice(free, n, replace=False))


def score_cases():
    rng = np.random.default_rng(POOL_SEED + 10)
    q = [None] * NQ
    q[0] = _normalised(rng, [])
    q[1] = _normalised(rng, [7])
    q[2] = _normalised(rng, 2 * _draw(rng, QUERY_LDS - 1, 0, ID_RANGE // 2))                           # even ids only
    q[3] = _normalised(rng, np.append(_draw(rng, QUERY_LDS - 1), TOP_ID))
    q[4] = _normalised(rng, _draw(rng, QUERY_LDS + 1, 100))
    q[5] = _normalised(rng, np.concatenate([[0, 7], _draw(rng, Q_CAP - 3, 8), [TOP_ID]]))
    q[6] = _normalised(rng, [])     # count -1: fixed_stride fills the whole slot with entries that must not be read
    db, patterns = [], {}

    def add(name, qi, vec):
        db.append(vec)
        patterns.setdefault(name, []).append((qi, len(db) - 1))

    add("identical", 5, (q[5][0].copy(), q[5][1].copy()))             # db[0]: what a one-column matrix holds
    add("identical", 1, (q[1][0].copy(), q[1][1].copy()))             # one entry of value 1 on both sides: exactly 1
    add("identical", 3, (q[3][0].copy(), q[3][1].copy()))
    add("disjoint", 2, _normalised(rng, _draw(rng, 300, ID_RANGE + 10000, ID_RANGE + 20000)))
    add("disjoint", 4, _normalised(rng, _draw(rng, QUERY_LDS + 1, ID_RANGE + 10000, ID_RANGE + 20000)))
    add("interleaved", 2, _normalised(rng, q[2][0] + 1))              # odd ids between the even ones
    add("interleaved", 5, _normalised(rng, _draw(rng, Q_CAP, 1, avoid=q[5][0])))
    i4, i5 = q[4][0].astype(np.int64), q[5][0].astype(np.int64)
    add("first", 4, _normalised(rng, np.append(i4[0], _draw(rng, 400, i4[0] + 1, avoid=i4))))
    add("first", 5, _normalised(rng, np.append(0, _draw(rng, QUERY_LDS, 1, avoid=i5))))
    add("last", 4, _normalised(rng, np.append(_draw(rng, 400, 0, i4[-1], avoid=i4), i4[-1])))
    add("last", 5, _normalised(rng, np.append(_draw(rng, Q_CAP - 1, 1, avoid=i5), TOP_ID)))
    add("long_vs_one", 5, _normalised(rng, [i5[4100]]))
    add("long_vs_one", 4, _normalised(rng, [i4[-1]]))
    add("one_vs_long", 1, _normalised(rng, np.union1d(_draw(rng, Q_CAP - 1, 8), [7])))
    add("extreme_ids", 5, _normalised(rng, [0, TOP_ID]))
    add("extreme_ids", 3, _normalised(rng, [TOP_ID]))
    add("empty", 5, _normalised(rng, []))
    while len(db) < NDB:            # a few hundred entries each; every other one holds the one-entry query's id
        ids = _draw(rng, int(rng.integers(100, 600)), 8)
        db.append(_normalised(rng, np.union1d(ids, [7]) if len(db) % 2 else ids))
    return ScoreCases(q, db, patterns)


DB_OVERFLOW = NDB - 2           # this database slot's count is -1 in the device layout: the expected scores take it as empty


def score_vectors(cases):
    """What the scores are defined on: the lists with the slots of count -1 replaced by empty vectors."""
    empty = (np.zeros(0, np.uint32), np.zeros(0, np.float64))
    db = list(cases.db)
    db[DB_OVERFLOW] = empty
    return list(cases.q), db


def expected_scores(cases):
    """[NQ, NDB] float64: the oracle's L1Scoring::score, pair by pair."""
    q, db = score_vectors(cases)
    return np.array([[po.score_l1(a, b) for b in db] for a in q], np.float64)


def fixed_stride(vectors, stride, overflow, seed):
    """The device layout: ids [n, stride] uint32, vals [n, stride] float64, counts [n] int32.  The slots past a count hold ascending ids that
    the other side holds too, with values that would change any score they entered; the vectors in `overflow` get the count -1 and keep
    their entries."""
    rng = np.random.default_rng(seed)
    n = len(vectors)
    ids = np.sort(rng.integers(0, ID_RANGE, (n, stride)).astype(np.uint32), axis=1)
    vals = rng.uniform(0.5, 2.0, (n, stride))
    counts = np.zeros(n, np.int32)
    for i, (a, v) in enumerate(vectors):
        ids[i, :len(a)] = a
        vals[i, :len(a)] = v
        counts[i] = -1 if i in overflow else len(a)
    return ids, vals, counts
