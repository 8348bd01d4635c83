"""A small numpy model of DBoW2's TemplatedVocabulary::create (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:558-616) after
DUtils::Random::SeedRandOnce(seed), with the two departures of include/orbx_train.h (an empty cluster keeps its previous centre; no
convergence within max_iterations raises).  Written from the reference's description, independent of liborbx_train.so: the CPU suite holds
it to the reference's goldens (tests/golden/voc_train.npz), the GPU suite holds the library to it on cases the reference cannot run."""
from __future__ import annotations

import math

import numpy as np

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
RAND_MAX = 2147483647


class GlibcRand:
    """glibc srand / rand (TYPE_3, random_r.c): r[i] = r[i-3] + r[i-31], output r >> 1, 310 discarded after seeding."""

    def __init__(self, seed: int):
        word = seed & 0xFFFFFFFF
        if word == 0:
            word = 1
        if word >= 1 << 31:
            word -= 1 << 32          # the state words are int32_t
        r = [word]
        for _ in range(30):
            hi, lo = int(word / 127773), word - int(word / 127773) * 127773   # C division truncates
            word = 16807 * lo - 2836 * hi
            if word < 0:
                word += 2147483647
            r.append(word)
        self.r = [x & 0xFFFFFFFF for x in r]
        self.f, self.b = 3, 0
        for _ in range(310):
            self.next()

    def next(self) -> int:
        v = (self.r[self.f] + self.r[self.b]) & 0xFFFFFFFF
        self.r[self.f] = v
        self.f = (self.f + 1) % 31
        self.b = (self.b + 1) % 31
        return v >> 1

    def random_int(self, lo: int, hi: int) -> int:          # DUtils::Random::RandomInt
        return int((self.next() / (RAND_MAX + 1.0)) * (hi - lo + 1)) + lo

    def random_value(self, lo: float, hi: float) -> float:  # DUtils::Random::RandomValue<double>
        return self.next() / float(RAND_MAX) * (hi - lo) + lo


class NoConvergence(RuntimeError):
    pass


def _popcount64(v: np.ndarray) -> np.ndarray:
    if hasattr(np, "bitwise_count"):
        return np.bitwise_count(v)
    return _POP[v.view(np.uint8).reshape(v.shape + (8,))].sum(-1)


def _dist(x: np.ndarray, c: np.ndarray) -> np.ndarray:
    """FORB::distance of every row of x (n, 32) to every centre c (m, 32): (n, m) int.  A bit count over four uint64 words per pair (the
    (n, m, 32) byte-table lookup takes minutes on 10^5 rows)."""
    xw = np.ascontiguousarray(x, np.uint8).reshape(-1, 32).view(np.uint64)
    cw = np.ascontiguousarray(c, np.uint8).reshape(-1, 32).view(np.uint64)
    out = np.zeros((len(xw), len(cw)), np.int64)
    for j in range(len(cw)):
        out[:, j] = _popcount64(xw ^ cw[j]).sum(1)
    return out


def _mean(x: np.ndarray) -> np.ndarray:
    """FORB::meanValue (FORB.cpp:28-77) of a non-empty group."""
    n = len(x)
    cnt = np.unpackbits(x, axis=1).sum(0)
    return np.packbits(cnt >= n // 2 + n % 2)


def create(desc: np.ndarray, offsets, k: int, L: int, weighting: int, seed: int, max_iterations: int = 10000, trace: list | None = None):
    """-> (parent, is_leaf, desc, weight) over all nodes, root (id 0) included, and {'empty_clusters', 'iterations'}.
    `trace`, when given, receives one dict per k-means node in the reference's depth-first order: level, n, first (the first centre's index),
    draws (one (n, sum, ceil(cut), chosen index) per k-means++ draw) and kc (the centres seeded)."""
    X = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    offsets = np.asarray(offsets, np.int64)
    rng = GlibcRand(seed)
    parent, ndesc = [0], [np.zeros(32, np.uint8)]
    stats = {"empty_clusters": 0, "iterations": 0}

    def kmeans(x, level):
        n = len(x)
        i0 = rng.random_int(0, n - 1)
        draws = []
        cents = [x[i0]]
        md = _dist(x, x[i0][None])[:, 0].astype(np.int64)
        while len(cents) < k:
            s = int(md.sum())
            if s == 0:
                break
            cut = 0.0
            while cut == 0.0:
                cut = rng.random_value(0.0, float(s))
            idx = int(np.searchsorted(np.cumsum(md), math.ceil(cut), side="left"))
            draws.append((n, s, math.ceil(cut), min(idx, n - 1)))
            cents.append(x[min(idx, n - 1)])
            md = np.minimum(md, _dist(x, x[min(idx, n - 1)][None])[:, 0])
        if trace is not None:
            trace.append({"level": level, "n": n, "first": i0, "draws": draws, "kc": len(cents)})
        c = np.array(cents, np.uint8)
        assoc = np.argmin(_dist(x, c), axis=1)   # argmin returns the first minimum: the strict < of the reference
        it = 1
        while True:
            if it >= max_iterations:
                raise NoConvergence(f"no convergence within {max_iterations}")
            for j in range(len(c)):
                g = x[assoc == j]
                if len(g) == 0:
                    stats["empty_clusters"] += 1
                else:
                    c[j] = _mean(g)
            new = np.argmin(_dist(x, c), axis=1)
            it += 1
            if np.array_equal(new, assoc):
                break
            assoc = new
        stats["iterations"] += it
        return c, assoc

    def step(pid, x, level):
        if len(x) == 0:
            return
        if len(x) <= k:
            c, assoc = x.copy(), np.arange(len(x))
        else:
            c, assoc = kmeans(x, level)
        first = len(parent)
        for j in range(len(c)):
            parent.append(pid)
            ndesc.append(c[j].copy())
        if level < L:
            for j in range(len(c)):
                g = x[assoc == j]   # boolean selection keeps the original order
                if len(g) > 1:
                    step(first + j, g, level + 1)

    step(0, X, 1)
    nn = len(parent)
    parent = np.array(parent, np.int32)
    leaf = np.ones(nn, np.uint8)
    leaf[parent[1:]] = 0
    leaf[0] = 1 if nn == 1 else 0
    D = np.array(ndesc, np.uint8)
    weight = np.zeros(nn, np.float64)
    words = np.nonzero(leaf[1:])[0] + 1
    if weighting in (1, 3):          # TF, BINARY
        weight[words] = 1.0
    else:                            # TF_IDF, IDF: ln(NDocs / Ni), Ni = documents that reach the word
        word_of = descend(parent, leaf, D, X)
        ndocs = len(offsets) - 1
        ni = {}
        for d in range(ndocs):
            for w in set(word_of[offsets[d]:offsets[d + 1]].tolist()):
                ni[w] = ni.get(w, 0) + 1
        for w, c in ni.items():
            weight[w] = math.log(float(ndocs) / float(c))
    return (parent, leaf, D, weight), stats


def descend(parent, leaf, D, X):
    """transform(feature, word_id) (TemplatedVocabulary.h:1262-1302) of every row: the leaf NODE id reached."""
    children = [[] for _ in range(len(parent))]
    for i in range(1, len(parent)):
        children[parent[i]].append(i)
    out = np.zeros(len(X), np.int64)   # every row starts at the root; a child's id is above its parent's, so one pass in id order descends all
    for nid in range(len(parent)):
        ch = children[nid]
        if not ch:
            continue
        rows = np.nonzero(out == nid)[0]
        if len(rows):
            out[rows] = np.array(ch, np.int64)[np.argmin(_dist(X[rows], D[ch]), axis=1)]
    return out
