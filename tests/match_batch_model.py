"""A plain statement of the batched SearchByBoW's semantics (include/orbx_match.h), both modes, written from the description of the loop:
what the GPU suite holds the library to where the oracle has no array-level routine (keyframe mode), and what counts contended B features.

FeatureVectors are dicts node -> list of feature indices (the list order is the scan order)."""
from __future__ import annotations

import math

import numpy as np

FRAME, KEYFRAMES = 0, 1
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
_F = np.float32


def rotation_bin(angle_a, angle_b) -> int:
    """The histogram bin of one match: float32 arithmetic, C's round (half away from zero), bin 30 wraps to 0."""
    rot = _F(angle_a) - _F(angle_b)
    if rot < 0:
        rot = _F(rot + _F(360.0))
    x = float(_F(rot * (_F(1.0) / _F(30))))
    b = int(math.copysign(math.floor(abs(x) + 0.5), x))
    return 0 if b == 30 else b


def three_maxima(sizes):
    """The (up to) three fullest bins: a second or third bin under a tenth of the first does not count."""
    ind, mx = [-1, -1, -1], [0, 0, 0]
    for i, s in enumerate(sizes):
        if s > mx[0]:
            mx, ind = [s, mx[0], mx[1]], [i, ind[0], ind[1]]
        elif s > mx[1]:
            mx, ind = [mx[0], s, mx[1]], [ind[0], i, ind[1]]
        elif s > mx[2]:
            mx[2], ind[2] = s, i
    if _F(mx[1]) < _F(0.1) * _F(mx[0]):
        ind[1] = ind[2] = -1
    elif _F(mx[2]) < _F(0.1) * _F(mx[0]):
        ind[2] = -1
    return ind


def search_by_bow(desc_a, angle_a, valid_a, fv_a, desc_b, angle_b, valid_b, fv_b, mode=FRAME, nn_ratio=0.7, check_orientation=True, stats=None):
    """(nmatches, b2a [len(desc_b)]): b2a[i] = the A feature matched to B feature i, -1 for none.  valid_a / valid_b: uint8 arrays or None (all
    valid); valid_b only counts in keyframe mode.  `stats`, a dict, receives "contended" (B features a later A feature's unrestricted best
    pointed at after they were taken) and "removed" (matches the rotation filter dropped)."""
    desc_a, desc_b = np.asarray(desc_a, np.uint8).reshape(-1, 32), np.asarray(desc_b, np.uint8).reshape(-1, 32)
    nb = len(desc_b)
    b2a = np.full(nb, -1, np.int64)
    usable_b = np.ones(nb, bool)
    if mode == KEYFRAMES and valid_b is not None:
        usable_b = np.asarray(valid_b).astype(bool).copy()
    limit = 50 if mode == FRAME else 49          # <= 50 in frame mode, < 50 between keyframes
    bins = [[] for _ in range(30)]
    contended = set()
    for node in sorted(set(fv_a) & set(fv_b)):
        cand = np.asarray(fv_b[node], np.int64)
        for ia in fv_a[node]:
            if valid_a is not None and not valid_a[ia]:
                continue
            dist = _POP[desc_b[cand] ^ desc_a[ia]].sum(1)
            free = usable_b[cand] & (b2a[cand] < 0)
            if len(cand) and (~free).any():
                open_d = np.where(usable_b[cand], dist, 256)
                j = int(np.argmin(open_d))
                if open_d[j] < 256 and b2a[cand[j]] >= 0:
                    contended.add(int(cand[j]))
            d = np.where(free, dist, 256)
            best1, best_idx, best2 = 256, -1, 256
            if len(d):
                j = int(np.argmin(d))                                  # the first minimum in list order (strict <)
                if d[j] < 256:
                    best1, best_idx = int(d[j]), int(cand[j])
                    rest = np.delete(d, j)                             # the second smallest is the smallest of the others, ties included
                    best2 = min(int(rest.min()), 256) if len(rest) else 256
            if best1 <= limit and _F(best1) < _F(nn_ratio) * _F(best2):
                b2a[best_idx] = ia
                if check_orientation:
                    b = rotation_bin(angle_a[ia], angle_b[best_idx])
                    if 0 <= b < 30:
                        bins[b].append(best_idx)
    removed = 0
    if check_orientation:
        keep = three_maxima([len(b) for b in bins])
        for i, members in enumerate(bins):
            if i not in keep:
                for ib in members:
                    b2a[ib] = -1
                    removed += 1
    if stats is not None:
        stats["contended"] = len(contended)
        stats["removed"] = removed
    return int((b2a >= 0).sum()), b2a.astype(np.int32)


def invert(b2a, na):
    """a2b of a b2a row."""
    a2b = np.full(na, -1, np.int32)
    hit = np.nonzero(np.asarray(b2a) >= 0)[0]
    a2b[np.asarray(b2a)[hit]] = hit
    return a2b
