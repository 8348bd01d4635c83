"""The six DBoW2 scorings (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp) restated in numpy float64, one rounded operation per statement:
what liborbx_score.so is held to (tests/test_score_model.py holds this file to the reference's own library first).

  score(scoring, a, b)        the reference's loops as they stand: the walk with its lower_bound jumps, KL's one-entry steps and tail loop
  score_terms(scoring, a, b)  the same additions found with array operations -- the terms in the order the walk adds them --, for the
                              large batches; score_fast sums them one after the other from 0 and applies the scoring's last line
A vector is (ids ascending and unique, values).  log is libm's (math.log: numpy's own vector log need not equal it), with C's results at 0,
below 0 and at NaN."""
import bisect
import math

import numpy as np

L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT = range(6)
F = np.float64
LOG_EPS = F(math.log(float(np.finfo(np.float64).eps)))     # GeneralScoring::LOG_EPS = log(DBL_EPSILON), ScoringObject.cpp:18


def c_log(x):
    """C's log(double)."""
    x = float(x)
    if x != x or x < 0.0:
        return F(np.nan)
    if x == 0.0:
        return F(-np.inf)
    if x == math.inf:
        return F(np.inf)
    return F(math.log(x))


def _vec(v):
    return [int(i) for i in np.asarray(v[0])], np.asarray(v[1], np.float64)


def _term(scoring, vi, wi):
    """What one common word adds under the five scorings that add per common word only; None: nothing."""
    if scoring == L1_NORM:
        d = vi - wi
        t = np.abs(d) - np.abs(vi)
        return t - np.abs(wi)
    if scoring == CHI_SQUARE:
        s = vi + wi
        if not (s != 0.0):
            return None
        p = vi * wi
        return p / s
    p = vi * wi
    return np.sqrt(p) if scoring == BHATTACHARYYA else p


def finish(scoring, score):
    """The scoring's last line."""
    if scoring == L1_NORM:
        return -score / F(2.0)
    if scoring == L2_NORM:
        if score >= 1:
            return F(1.0)
        r = F(1.0) - score
        return F(1.0) - np.sqrt(r)
    if scoring == CHI_SQUARE:
        return F(2.0) * score
    return score


def score(scoring, a, b):
    """TemplatedVocabulary::score under `scoring`, the reference's loop."""
    (ia, va), (ib, vb) = _vec(a), _vec(b)
    na, nb = len(ia), len(ib)
    x = y = 0
    s = F(0.0)
    with np.errstate(all="ignore"):
        if scoring == KL:
            while x < na and y < nb:
                vi, wi = va[x], vb[y]
                if ia[x] == ib[y]:
                    if vi != 0 and wi != 0:
                        r = vi / wi
                        t = vi * c_log(r)
                        s = s + t
                    x += 1
                    y += 1
                elif ia[x] < ib[y]:
                    d = c_log(vi) - LOG_EPS
                    t = vi * d
                    s = s + t
                    x += 1
                else:
                    y = bisect.bisect_left(ib, ia[x], y)
            while x < na:
                if va[x] != 0:
                    d = c_log(va[x]) - LOG_EPS
                    t = va[x] * d
                    s = s + t
                x += 1
            return F(s)
        while x < na and y < nb:
            if ia[x] == ib[y]:
                t = _term(scoring, va[x], vb[y])
                if t is not None:
                    s = s + t
                x += 1
                y += 1
            elif ia[x] < ib[y]:
                x = bisect.bisect_left(ia, ib[y], x)
            else:
                y = bisect.bisect_left(ib, ia[x], y)
        return F(finish(scoring, s))


def score_terms(scoring, a, b):
    """The terms the walk adds, in its order (float64 array)."""
    ia, va = np.asarray(a[0], np.uint32), np.asarray(a[1], np.float64)
    ib, vb = np.asarray(b[0], np.uint32), np.asarray(b[1], np.float64)
    _, xa, xb = np.intersect1d(ia, ib, assume_unique=True, return_indices=True)    # ascending id
    vi, wi = va[xa], vb[xb]
    with np.errstate(all="ignore"):
        if scoring == L1_NORM:
            d = vi - wi
            t = np.abs(d) - np.abs(vi)
            return t - np.abs(wi)
        if scoring == CHI_SQUARE:
            s = vi + wi
            p = vi * wi
            return (p / s)[s != 0.0]
        if scoring in (L2_NORM, DOT_PRODUCT):
            return vi * wi
        if scoring == BHATTACHARYYA:
            p = vi * wi
            return np.sqrt(p)
        # KL: every entry of the first vector has its place in the order.  A word the second vector lacks is met in the walk (no test
        # of its value) while the second vector still has a larger id, and in the tail loop (value != 0 only) after that
        n = len(ia)
        logv = np.array([c_log(v) for v in va], np.float64)
        d = logv - LOG_EPS
        t = va * d
        tail = ia > ib[-1] if len(ib) else np.ones(n, bool)
        keep = ~tail | (va != 0)
        r = vi / wi
        t[xa] = vi * np.array([c_log(v) for v in r], np.float64)
        keep[xa] = (vi != 0) & (wi != 0)
        return t[keep]


def sequential_sum(terms):
    """0 + t0 + t1 + ..., each addition rounded, in order."""
    return F(np.cumsum(np.concatenate([[0.0], np.asarray(terms, np.float64)]))[-1])


def score_fast(scoring, a, b):
    with np.errstate(all="ignore"):
        return F(finish(scoring, sequential_sum(score_terms(scoring, a, b))))


def pairwise_sum(terms):
    """The same terms added as a balanced tree: another order of the same additions."""
    t = [F(x) for x in terms]
    if not t:
        return F(0.0)
    while len(t) > 1:
        t = [t[i] + t[i + 1] if i + 1 < len(t) else t[i] for i in range(0, len(t), 2)]
    return t[0]


def fma(a, b, c):
    """a * b + c rounded once, exactly (rational arithmetic on finite doubles)."""
    from fractions import Fraction
    return F(float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))))


def dot_fused_at(a, b, k):
    """DOT_PRODUCT with the k-th common word's product fused into its addition (what a contracting compiler would make of it)."""
    t_ids, xa, xb = np.intersect1d(np.asarray(a[0], np.uint32), np.asarray(b[0], np.uint32), assume_unique=True, return_indices=True)
    vi, wi = np.asarray(a[1], np.float64)[xa], np.asarray(b[1], np.float64)[xb]
    s = F(0.0)
    for j in range(len(t_ids)):
        if j == k:
            s = fma(vi[j], wi[j], s)
        else:
            p = vi[j] * wi[j]
            s = s + p
    return s


def same_bits(x, y):
    """Equal as results: both NaN, or the same 64 bits."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return (np.isnan(x) & np.isnan(y)) | (x.view(np.uint64) == y.view(np.uint64))
