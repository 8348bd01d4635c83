"""tests/initmatch_model.py (the three phases of liborbx_initmatch.so's kernel, in Python) against the oracle's
ORBmatcher::SearchForInitialization: on extracted frames over the parameters, and on hand cases for every point of the specification a
parallel restatement can get wrong (include/orbx_initmatch.h).  CPU only."""
import functools
import itertools

import numpy as np
import pytest

from oracle import pyoracle as po
from orb_slam3_modified_amd import synth
from orb_slam3_modified_amd._lib import KP_DTYPE
from tests import initmatch_model as im

EXTRACTORS = {"euroc1000": (480, 752, (1000, 1.2, 8, 20, 7)), "vga5000": (480, 640, (5000, 1.2, 8, 20, 7)), "onelevel": (480, 752, (1000, 1.2, 1, 20, 7))}
COMBOS = list(itertools.product((30, 100, 200), (0.6, 0.9), (True, False), (False, True)))   # window, ratio, orientation, bounds beyond the image


@functools.lru_cache(maxsize=None)
def _frames(name):
    H, W, cfg = EXTRACTORS[name]
    ex = po.OracleExtractor(*cfg)
    out = []
    for img in synth.make_stream(7, H, W):
        kps, desc, _ = ex.extract(img, (0, 1000))
        out.append((kps, desc))
    return out, (H, W)


def _bounds(H, W, beyond):
    return (-20.5, -10.25, W + 31.5, H + 17.75) if beyond else (0.0, 0.0, float(W), float(H))


def _both(k1, d1, k2, d2, bounds, prev, window, ratio, ori, stats=None):
    """The model's result, held to the oracle's: matches12, the count and prev as bytes."""
    p0 = np.stack([k1["x"], k1["y"]], 1).astype(np.float32) if prev is None else np.asarray(prev, np.float32)
    on, om12, oprev = po.search_for_initialization(k1, d1, k2, d2, bounds, p0, window, ratio, ori)
    mn, mm12, mprev = im.search_for_initialization(k1, d1, k2, d2, bounds, p0, window, ratio, ori, stats=stats)
    assert mn == on and np.array_equal(mm12, om12) and mprev.tobytes() == oprev.tobytes(), (mn, on, window, ratio, ori)
    if prev is None:     # "no prev": F1's own positions as centres give the same matches
        nn, nm12, nprev = im.search_for_initialization(k1, d1, k2, d2, bounds, None, window, ratio, ori)
        assert nn == on and np.array_equal(nm12, om12) and nprev is None
    return on, om12, oprev


@pytest.mark.parametrize("name", list(EXTRACTORS))
def test_model_equals_oracle_on_extracted_frames(name):
    frames, (H, W) = _frames(name)
    level0 = [(k["octave"] == 0).sum() for k, _ in frames]
    if name == "onelevel":
        assert all(n == len(k) > 500 for n, (k, _) in zip(level0, frames))     # every feature is level 0
    else:
        assert all(0 < n < len(k) for n, (k, _) in zip(level0, frames))
    pairs = [(0, 1), (0, 5), (3, 3)]
    stats_on, stats_off, total = {}, {}, 0
    for i, (window, ratio, ori, beyond) in enumerate(COMBOS):
        if name == "vga5000" and i % 3 != 0:        # the long lists: a third of the combinations, every window and both ratios among them
            continue
        fa, fb = pairs[i % 3]
        (k1, d1), (k2, d2) = frames[fa], frames[fb]
        n, _, _ = _both(k1, d1, k2, d2, _bounds(H, W, beyond), None, window, ratio, ori, stats_on if ori else stats_off)
        total += n
    # F1 chained against two successive frames with prev carried over (src/Tracking.cc:2470-2495 over two frames)
    for window, ratio, ori, beyond in ((100, 0.9, True, False), (30, 0.6, False, True)):
        k1, d1 = frames[0]
        prev = None
        for f in (1, 2):
            k2, d2 = frames[f]
            n, _, prev = _both(k1, d1, k2, d2, _bounds(H, W, beyond), prev, window, ratio, ori, stats_on if ori else stats_off)
        assert n > 0
    # F2 = F1 with a shifted prev: every window holds its neighbours' features first
    k1, d1 = frames[2]
    shifted = np.stack([k1["x"] + 7.5, k1["y"] - 4.25], 1).astype(np.float32)
    _both(k1, d1, k1, d1, _bounds(H, W, False), shifted, 100, 0.9, True, stats_on)
    assert total > 100
    for st in (stats_on, stats_off):
        assert st["steals"] > 0 and st["skipped_taken"] > 0, (name, st)
    assert stats_on["removed"] > 0, (name, stats_on)


# ---- hand cases: bounds 640 x 480, so a cell is 10 x 10 pixels; desc(k) has its k leading bits set, so |a - b| is the distance
B640 = (0.0, 0.0, 640.0, 480.0)


def desc(k):
    d = np.zeros(32, np.uint8)
    d[:k // 8] = 0xFF
    if k % 8:
        d[k // 8] = (0xFF << (8 - k % 8)) & 0xFF
    return d


def frame(points):
    """points: (x, y, descriptor bits[, angle[, octave]]) -> (keypoints, descriptors)."""
    k = np.zeros(len(points), KP_DTYPE)
    d = np.zeros((len(points), 32), np.uint8)
    for i, p in enumerate(points):
        k["x"][i], k["y"][i] = p[0], p[1]
        d[i] = desc(p[2])
        k["angle"][i] = p[3] if len(p) > 3 else 0.0
        k["octave"][i] = p[4] if len(p) > 4 else 0
        k["size"][i] = 31.0
    return k, d


def run(f1, f2, window=30, ratio=0.9, ori=False, prev=None, stats=None):
    n, m12, pv = _both(*f1, *f2, B640, prev, window, ratio, ori, stats)
    assert n == (m12 >= 0).sum()
    return m12.tolist(), pv


def test_a_closer_later_query_steals():
    st = {}
    m12, prev = run(frame([(100, 100, 10), (102, 100, 3)]), frame([(101, 100, 0)]), stats=st)
    assert m12 == [-1, 0] and st["steals"] == 1
    assert prev.tolist() == [[100.0, 100.0], [101.0, 100.0]]     # the robbed query's prev row is untouched


def test_equal_distance_does_not_steal():
    st = {}
    m12, _ = run(frame([(100, 100, 10), (102, 100, 10)]), frame([(101, 100, 0)]), stats=st)
    assert m12 == [0, -1] and st["steals"] == 0 and st["skipped_taken"] == 1


def test_a_tie_goes_to_the_first_candidate_in_grid_order():
    # F2 index 0 lies in cell (11, 10), indices 1 and 2 in cell (9, 10): the grid's order is 1, 2, 0
    f2 = frame([(112, 100, 5), (93, 100, 5), (94, 101, 5)])
    m12, _ = run(frame([(100, 100, 0)]), f2, ratio=1.5)
    assert m12 == [1]
    m12, _ = run(frame([(100, 100, 0)]), frame([(112, 100, 5), (94, 101, 5), (93, 100, 5)]), ratio=1.5)
    assert m12 == [1]                                           # inside a cell: ascending index
    m12, _ = run(frame([(100, 100, 0)]), f2, ratio=0.9)
    assert m12 == [-1]                                          # the tie is the second best too


def test_th_low_is_inclusive():
    assert run(frame([(100, 100, 50)]), frame([(101, 100, 0)]))[0] == [0]
    assert run(frame([(100, 100, 51)]), frame([(101, 100, 0)]))[0] == [-1]


def test_ratio_boundary():
    f2 = frame([(101, 100, 0), (103, 100, 5)])               # distances to desc(10): 10 and 5; to desc(11): 11 and 6 ...
    assert run(frame([(100, 100, 10)]), f2, ratio=0.5)[0] == [-1]      # 5 < 10 * 0.5 is false at equality
    assert run(frame([(100, 100, 10)]), frame([(101, 100, 0), (103, 100, 6)]), ratio=0.5)[0] == [1]   # 4 < 5.0


def test_a_single_candidate_meets_int_max():
    st = {}
    assert run(frame([(100, 100, 30)]), frame([(101, 100, 0)]), ratio=0.1, stats=st)[0] == [0]   # 30 < 2147483648 * 0.1, not 30 < 25.6
    assert st["single_candidate"] == 1


def test_the_window_is_open():
    assert run(frame([(100, 100, 0)]), frame([(130, 100, 0)]), window=30)[0] == [-1]
    assert run(frame([(100, 100, 0)]), frame([(129.5, 100, 0)]), window=30)[0] == [0]
    assert run(frame([(100, 100, 0)]), frame([(100, 70, 0)]), window=30)[0] == [-1]


@pytest.mark.parametrize("px,py", [(-25.0, 100.0), (670.0, 100.0), (100.0, -25.0), (100.0, 505.0)])
def test_prev_outside_the_grid_has_no_candidates(px, py):
    f2 = frame([(1, 100, 0), (639, 100, 0), (100, 1, 0), (100, 479, 0)])
    m12, prev = run(frame([(100, 100, 0)]), f2, window=10, prev=np.array([[px, py]], np.float32))
    assert m12 == [-1] and prev.tolist() == [[px, py]]


def test_only_level_zero_on_both_sides():
    f1 = frame([(100, 100, 0, 0.0, 1), (200, 100, 0), (300, 100, 0, 0.0, 3)])
    f2 = frame([(100, 100, 0), (200, 100, 0, 0.0, 1), (201, 100, 7), (300, 100, 0, 0.0, 2)])
    assert run(f1, f2)[0] == [-1, 2, -1]


def _spread(rows):
    """One query and one F2 feature per row, 60 pixels apart: with window 10 each query sees its own feature alone."""
    return (frame([(50 + 60 * i, 100, 0, a) for i, a in enumerate(rows)]), frame([(50 + 60 * i, 100, 0, 0.0) for i in range(len(rows))]))


def test_bin_30_folds_to_0():
    # rot 900 -> bin 30 -> 0: bins 0, 3, 6 hold two matches each and win; without the fold bin 9 would be among the three
    f1, f2 = _spread([900.0, 900.0, 90.0, 90.0, 180.0, 180.0, 270.0])
    st = {}
    assert run(f1, f2, window=10, ori=True, stats=st)[0] == [0, 1, 2, 3, 4, 5, -1] and st["removed"] == 1
    assert im.rot_bin(900.0, 0.0) == 0


def test_a_stolen_acceptance_stays_in_the_histogram():
    # query 0 (bin 9) is accepted with F2 feature 0 and robbed by query 1 (bin 0).  Counted, bin 9 holds 2 and beats bin 6's 1: query 5 loses
    # its match.  Were the stolen acceptance taken out again, bin 6 would win and query 6 would lose instead.
    f1 = frame([(50, 100, 10, 270.0), (51, 100, 3, 0.0), (110, 100, 0, 0.0), (170, 100, 0, 90.0), (230, 100, 0, 90.0), (290, 100, 0, 180.0),
                (350, 100, 0, 270.0)])
    f2 = frame([(50, 100, 0), (110, 100, 0), (170, 100, 0), (230, 100, 0), (290, 100, 0), (350, 100, 0)])
    st = {}
    assert run(f1, f2, window=10, ori=True, stats=st)[0] == [-1, 0, 1, 2, 3, -1, 5]
    assert st["steals"] == 1 and st["removed"] == 1
    assert run(f1, f2, window=10, ori=False)[0] == [-1, 0, 1, 2, 3, 4, 5]
