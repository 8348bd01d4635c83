"""One constructed batch for the batched SearchForInitialization (include/orbx_initmatch.h): 16 pairs over 18 small frames, capacity 256.
Every edge of the specification is planted at a site of its own; where an edge has two sides both are planted ("at" / "over"), so that a
wrong comparison flips exactly one named outcome.  numpy only: the CPU test (tests/test_initmatch_model.py) holds the batch to its claims on
tests/initmatch_model.py and the oracle, the GPU test (tests/test_gpu_initmatch.py) runs it through the kernel on every path.

A call has one window, one nn_ratio and one set of bounds for all its pairs, so the batch comes with RUNS: every pair goes through every
run (whole rows against the oracle), and a site's claim names the run it was built for.  Pairs whose frames carry angle 0 throughout are
untouched by check_orientation (one bin); the rotation sites live in pairs of their own.

PLANTED[name] = the query (index in the pair's F1 frame), KP[name] = the F2 feature the site is about (index in the F2 frame),
CLAIMS[name] = (pair, run, what the query holds after the run given prev_xy: a KP name or None, the same for prev_xy = NULL).

The frame count is above the handful one would wish for: F2's in-grid level-0 count n0 has to be 0, 1, 2, 64, 65 and 130+, each count is a
frame, and the three two-trip lists need 130 keypoints of one window each."""
import numpy as np

from orb_slam3_modified_amd._lib import KP_DTYPE
from tests import initmatch_model as im

F32 = np.float32
CAP = 256
WINDOW = 10
B640 = (0.0, 0.0, 640.0, 480.0)                                  # a cell is 10 x 10 pixels
BEYOND = (-20.5, -10.25, 640 + 31.5, 480 + 17.75)                # tests/test_gpu_initmatch.py::_bounds(beyond): invW, invH are not representable
(PLANT1, PLANT2, ROTA, ROTB, ROT2, QA, DENSE_A, DENSE_B, DENSE_C, MANYQ, BEY1, BEY2, FULL, EMPTY, NOLEVEL0, TWO, NEG, OVER) = range(18)
K = 18
# the pairs; 2, 7 and 12 are malformed, one of each kind the header lists
P_PLANT, P_ROTA, P_BADFRAME, P_ROTB, P_LANE, P_TWIN, P_MANY, P_BADCOUNT, P_BEY, P_FULL, P_NOA, P_NOB, P_OVER, P_NOLEVEL0, P_ONE, P_TWO = range(16)
PAIRS = np.array([(PLANT1, PLANT2), (ROTA, ROT2), (PLANT1, K), (ROTB, ROT2), (QA, DENSE_B), (QA, DENSE_C), (MANYQ, DENSE_A), (NEG, PLANT2),
                  (BEY1, BEY2), (FULL, FULL), (EMPTY, PLANT2), (PLANT1, EMPTY), (PLANT1, OVER), (PLANT1, NOLEVEL0), (QA, QA), (QA, TWO)], np.int32)
MALFORMED = {P_BADFRAME: "frame", P_BADCOUNT: "negative count", P_OVER: "count above capacity"}
N0 = {ROT2: 64, QA: 1, DENSE_A: 132, DENSE_B: 130, DENSE_C: 130, FULL: 65, EMPTY: 0, NOLEVEL0: 0, TWO: 2}   # in-grid level-0 counts


def ratio_triple():
    """(best, second, nn_ratio): float32(second) * float32(nn_ratio) rounds to exactly `best` although the product is above it -- the ratio
    test `best < second * nn_ratio` fails in float32 and would pass in double.  Found, not written down."""
    for r in (0.9, 0.8, 0.7, 0.6):
        for second in range(256, 1, -1):
            p = F32(second) * F32(r)
            if float(p) == int(p) and 30 <= int(p) <= im.TH_LOW and float(F32(second)) * float(F32(r)) > float(p):
                return int(p), second, r
    raise AssertionError("no triple")


BEST, SECOND, RATIO = ratio_triple()
# name -> (window_size, nn_ratio, bounds)
RUNS = {"main": (WINDOW, RATIO, B640), "low": (WINDOW, 0.1, B640), "high": (WINDOW, 1.5, B640), "beyond": (WINDOW, 1.5, BEYOND)}


def desc(k):
    """A descriptor with its k leading bits set: |a - b| is the distance of desc(a) and desc(b)."""
    d = np.zeros(32, np.uint8)
    d[:k // 8] = 0xFF
    if k % 8:
        d[k // 8] = (0xFF << (8 - k % 8)) & 0xFF
    return d


def flip(d, lo, hi):
    """d with its bits lo .. hi - 1 flipped."""
    bits = np.unpackbits(np.asarray(d, np.uint8))
    bits[lo:hi] ^= 1
    return np.packbits(bits)


def bin_edge(lo_bin):
    """The largest float32 rotation that still falls into bin `lo_bin`, and its successor in bin lo_bin + 1 (against angle 0)."""
    a, b = F32(30 * lo_bin), F32(30 * lo_bin + 30)
    assert im.rot_bin(a, 0.0) == lo_bin and im.rot_bin(b, 0.0) == lo_bin + 1
    while np.nextafter(a, b) < b:
        mid = F32((float(a) + float(b)) / 2)
        if mid == a or mid == b:
            break
        if im.rot_bin(mid, 0.0) == lo_bin:
            a = mid
        else:
            b = mid
    return a, np.nextafter(a, F32(1e9))


def half_position(bounds, axis, k):
    """A float32 coordinate whose grid position under `bounds` is exactly k + 0.5 in the specification's arithmetic, or None."""
    lo, span, n = F32(bounds[axis]), F32(F32(bounds[axis + 2]) - F32(bounds[axis])), (im.COLS, im.ROWS)[axis]
    inv = F32(n) / span
    v = F32((k + 0.5) / float(inv) + float(lo))
    for cand in [v] + [np.nextafter(v, F32(s * 1e9)) for s in (-1, 1)]:
        if float(F32(F32(cand - lo) * inv)) == k + 0.5:
            return cand
    for s in (-1, 1):                                            # a few more neighbours
        cand = v
        for _ in range(8):
            cand = np.nextafter(cand, F32(s * 1e9))
            if float(F32(F32(cand - lo) * inv)) == k + 0.5:
                return cand
    return None


class _Frame:
    def __init__(self):
        self.kps, self.desc, self.n = np.zeros(CAP, KP_DTYPE), np.zeros((CAP, 32), np.uint8), 0

    def add(self, x, y, d, angle=0.0, octave=0):
        i = self.n
        assert i < CAP
        k = self.kps[i]
        k["x"], k["y"], k["angle"], k["octave"], k["size"] = x, y, angle, octave, 31.0
        self.desc[i] = desc(d) if np.isscalar(d) else d
        self.n += 1
        return i


def site(s):
    """Regular sites, 40 pixels apart: no window of 10 reaches from one into another."""
    return F32(30 + 40 * (s % 15)), F32(70 + 40 * (s // 15))


def build():
    """-> dict(kps [K, CAP], desc [K, CAP, 32], counts [K, 2], pairs [16, 2], prev [16, CAP, 2]) and fills PLANTED / KP / CLAIMS.
    prev is every query's own position except where a site moves it; rows past the count hold a pattern."""
    fr = [_Frame() for _ in range(K)]
    PLANTED.clear(); KP.clear(); CLAIMS.clear()
    moved = {}                                                   # (pair, query) -> prev centre
    nxt = lambda v, to: np.nextafter(F32(v), F32(to))   # noqa: E731

    def claim(name, pair, run, q, kp, want=True, want_noprev=None):
        PLANTED[name], KP[name] = q, kp
        w = name if want else None
        CLAIMS[name] = (pair, run, w, w if want_noprev is None else (name if want_noprev else None))

    P1, P2 = fr[PLANT1], fr[PLANT2]
    s = iter(range(200))
    # ---- (a) grid positions at exactly .5 decide the cell, and with it the order of a tie (run "high": a tie is accepted).  A at cell
    # position 12.5 goes to cell 13, B (higher index) lies in cell 12: B stands first.  One ulp below, A is in cell 12 too and wins by index.
    for name, axis, under in (("half_x", 0, False), ("half_x_under", 0, True), ("half_y", 1, False), ("half_y_under", 1, True)):
        c = list(site(next(s)))                                  # the site's coordinates are whole cells: c + 5 is a cell position of .5
        pa, pb, qc = list(c), list(c), list(c)
        pa[axis], pb[axis], qc[axis] = nxt(c[axis] + 5, 0) if under else F32(c[axis] + 5), F32(c[axis] + 3), F32(c[axis] + 4)
        a = P2.add(pa[0], pa[1], 5)
        b = P2.add(pb[0], pb[1], 5)
        claim(name, P_PLANT, "high", P1.add(qc[0], qc[1], 0), a if under else b)
        KP[name + ":a"], KP[name + ":b"] = a, b
    # positions -0.5, 63.5 and 47.5 round out of the grid: in no cell, although a window covers them; one ulp inside they match
    for name, x, y, qx, qy in (("neg_half_x", -5.0, 100.0, 2.0, 100.0), ("neg_half_x_in", nxt(-5.0, 0), 140.0, 2.0, 140.0),
                               ("hi_half_x", 635.0, 100.0, 630.0, 100.0), ("hi_half_x_in", nxt(635.0, 0), 140.0, 630.0, 140.0),
                               ("neg_half_y", 300.0, -5.0, 300.0, 2.0), ("neg_half_y_in", 340.0, nxt(-5.0, 0), 340.0, 2.0),
                               ("hi_half_y", 300.0, 475.0, 300.0, 470.0), ("hi_half_y_in", 340.0, nxt(475.0, 0), 340.0, 470.0)):
        claim(name, P_PLANT, "main", P1.add(qx, qy, 0), P2.add(x, y, 0), name.endswith("_in"))
    # ---- (b) octaves: F2 features of octave 1 and -1 are no candidates though they are the closest; queries of those octaves keep -1
    cx, cy = site(next(s))
    P2.add(cx + 1, cy, 20, octave=1); P2.add(cx - 1, cy, 20, octave=-1)
    claim("oct_f2", P_PLANT, "main", P1.add(cx, cy, 20), P2.add(cx, cy + 1, 0))
    for name, o in (("oct_q1", 1), ("oct_qneg", -1)):
        cx, cy = site(next(s))
        claim(name, P_PLANT, "main", P1.add(cx, cy, 0, octave=o), P2.add(cx + 1, cy, 0), False)
    # ---- (c) the window is open: |dx| == r is outside, the float below it inside; the same in y
    for name, axis, at in (("win_at_x", 0, True), ("win_in_x", 0, False), ("win_at_y", 1, True), ("win_in_y", 1, False)):
        cx, cy = site(next(s))
        p = [cx, cy]
        p[axis] = F32(p[axis] + WINDOW) if at else nxt(p[axis] + WINDOW, 0)
        claim(name, P_PLANT, "main", P1.add(cx, cy, 0), P2.add(p[0], p[1], 0), not at)
    # ---- (e) bestDist 50 is accepted, 51 is not
    for name, d in (("th_50", 50), ("th_51", 51)):
        cx, cy = site(next(s))
        claim(name, P_PLANT, "main", P1.add(cx, cy, d), P2.add(cx + 1, cy, 0), d <= 50)
    # ---- (f) the ratio at float32 equality is rejected, one bit closer is accepted
    for name, d in (("ratio_at", BEST), ("ratio_under", BEST - 1)):
        cx, cy = site(next(s))
        kp = P2.add(cx + 1, cy, d)
        P2.add(cx - 1, cy, SECOND)
        claim(name, P_PLANT, "main", P1.add(cx, cy, 0), kp, d < BEST)
    # ---- (g) one surviving candidate meets INT_MAX: accepted at nn_ratio 0.1 with distance 30 (run "low") ...
    cx, cy = site(next(s))
    claim("single", P_PLANT, "low", P1.add(cx, cy, 30), P2.add(cx + 1, cy, 0))
    # ... and with two candidates, one of them held by an earlier query at distance 0: skipped, not the second best either
    cx, cy = site(next(s))
    x = P2.add(cx + 1, cy, 0)
    claim("single_holder", P_PLANT, "low", P1.add(cx, cy, 0), x)
    claim("single_skipped", P_PLANT, "low", P1.add(cx, cy + 1, 30), P2.add(cx - 1, cy, 60))
    # ---- (h) a strictly closer later query steals; an equal one does not; a chain of three
    cx, cy = site(next(s))
    kp = P2.add(cx + 1, cy, 0)
    claim("robbed", P_PLANT, "main", P1.add(cx, cy, 10), kp, False)
    claim("steals", P_PLANT, "main", P1.add(cx + 2, cy, 3), kp)
    cx, cy = site(next(s))
    kp = P2.add(cx + 1, cy, 0)
    claim("keeps", P_PLANT, "main", P1.add(cx, cy, 10), kp)
    claim("equal_later", P_PLANT, "main", P1.add(cx + 2, cy, 10), kp, False)
    cx, cy = site(next(s))
    kp = P2.add(cx + 1, cy, 0)
    claim("chain_1", P_PLANT, "main", P1.add(cx, cy, 10), kp, False)
    claim("chain_2", P_PLANT, "main", P1.add(cx + 2, cy, 6), kp, False)
    claim("chain_3", P_PLANT, "main", P1.add(cx + 1, cy + 1, 3), kp)
    # ---- (i) a tie: the lower grid column stands first although it holds the higher index; inside a cell the ascending index; with
    # nn_ratio < 1 the tie is the second best too
    cx, cy = site(next(s))
    P2.add(cx + 8, cy, 5)                                        # cx is a whole cell: cx + 8 rounds one column up, cx - 7 one down
    kp = P2.add(cx - 7, cy, 5)
    claim("tie_columns", P_PLANT, "high", P1.add(cx, cy, 0), kp)
    claim("tie_columns_ratio", P_PLANT, "main", PLANTED["tie_columns"], kp, False)
    KP["tie_columns:higher_column"] = kp - 1
    cx, cy = site(next(s))
    kp = P2.add(cx + 1, cy + 1, 5)
    P2.add(cx + 2, cy, 5)
    claim("tie_cell", P_PLANT, "high", P1.add(cx, cy, 0), kp)
    # ---- prev_xy moves a window onto a feature the query's own position does not reach
    cx, cy = site(next(s))
    q = P1.add(cx, cy, 0)
    cx, cy = site(next(s))
    claim("prev_moves", P_PLANT, "main", q, P2.add(cx + 1, cy, 0), True, False)
    moved[P_PLANT, q] = (cx, cy)
    # ---- (d) the four early returns of GetFeaturesInArea: a centre outside the grid on each side, a feature in the nearest border cell.
    # The distance test alone already refuses that feature, so each return has a twin one cell inside, which matches.
    for name, own, centre, kpos, inside in (
            ("ret_min_x", (610, 200), (655, 300), (634, 300), False), ("ret_min_x_in", (610, 240), (640, 340), (634, 340), True),
            ("ret_max_x", (12, 200), (-25, 300), (-4, 300), False), ("ret_max_x_in", (12, 240), (-12, 340), (-4, 340), True),
            ("ret_min_y", (160, 455), (200, 495), (200, 474), False), ("ret_min_y_in", (120, 455), (240, 480), (240, 474), True),
            ("ret_max_y", (160, 20), (200, -25), (200, -4), False), ("ret_max_y_in", (120, 20), (240, -12), (240, -4), True)):
        q = P1.add(own[0], own[1], 0)
        claim(name, P_PLANT, "main", q, P2.add(kpos[0], kpos[1], 0), inside, False)
        moved[P_PLANT, q] = centre

    # ---- (m) rotation.  The bin is round(rot * (1.0f / 30)): a rotation below 360 reaches bin 12 at most (345 is bin 11's edge to bin 12),
    # and the fold of bin 30 to 0 takes a rotation of 885 or more, an angle no extractor writes; it is planted with 900.
    # ROT2: 64 isolated features (n0 = 64), angle 0 but where a site needs a negative difference
    e11, e12 = bin_edge(11)
    R2 = fr[ROT2]
    for i in range(64):
        R2.add(*site(i), 0, angle={40: 5.0, 42: 20.0}.get(i, 0.0))
    # pair P_ROTA: bin sizes 30, 3, 2, 1.  float32 0.1f * 30 is 3.0: the 3 stays, the 2 goes; the lone bin 11 is none of the three
    A = fr[ROTA]
    for i in range(30):
        q = A.add(*site(i), 0, angle=0.0)
    claim("rot_bin0", P_ROTA, "main", q, 29)
    for name, i, a, keep in (("rot_negative", 40, 0.0, True), ("rot_at_edge", 41, e12, True), ("rot_negative_2", 42, 10.0, True), ("rot_two_a", 43, 180.0, False),
                             ("rot_two_b", 44, 180.0, False), ("rot_under_edge", 45, e11, False)):
        claim(name, P_ROTA, "main", A.add(*site(i), 0, angle=a), i, keep)
    # pair P_ROTB: four bins of two.  Bin 0 is a rotation of 900 (bin 30 -> 0) and an acceptance that is stolen later; the strict > keeps
    # bins 0, 3, 6 and drops bin 9.  Without the fold or without the stolen entry bin 0 holds one, bin 9 is kept and the fold's match goes.
    Bq = fr[ROTB]
    claim("rot_fold", P_ROTB, "main", Bq.add(*site(0), 0, angle=900.0), 0)
    cx, cy = site(1)
    claim("rot_robbed", P_ROTB, "main", Bq.add(cx, cy, 10, angle=0.0), 1, False)
    claim("rot_robber", P_ROTB, "main", Bq.add(cx + 1, cy, 3, angle=90.0), 1)
    for name, i, a, keep in (("rot_3", 2, 90.0, True), ("rot_6a", 3, 180.0, True), ("rot_6b", 4, 180.0, True), ("rot_9a", 5, 270.0, False), ("rot_9b", 6, 270.0, False)):
        claim(name, P_ROTB, "main", Bq.add(*site(i), 0, angle=a), i, keep)

    # ---- (j) 130 level-0 features in one cell (the list order is the index order), one window over them: three lane trips
    def dense(f, n, special):
        for p in range(n):
            fr[f].add(F32(316 + p % 8), F32(236 + (p // 8) % 8), special.get(p, 100 + p % 50))
    tail = flip(np.zeros(32, np.uint8), 128, 228)                # 100 bits at the far end: far from every desc(k) of the cluster
    dense(DENSE_A, 132, {5: 20, 67: 20, 100: tail})
    dense(DENSE_B, 130, {7: 20, 71: 22})
    dense(DENSE_C, 130, {7: 20, 71: 100})
    q = fr[QA].add(320.0, 240.0, 0)
    # best (position 7) and second (position 71) on one lane, nothing else within the ratio: rejected; the second made farther: accepted
    claim("lane_pair", P_LANE, "main", q, 7, False)
    claim("lane_pair_twin", P_TWIN, "main", q, 7)
    # ---- (k) more than 64 queries: 0 .. 62 see nothing, 63 is accepted with feature 100 at distance 10, 64 steals it at distance 3 -- with a
    # room of one longest list (256) the two 132-candidate lists fall into different chunks, and 64 is the first query of the second group
    M = fr[MANYQ]
    for i in range(63):
        M.add(F32(20 + 9 * i), 50.0, 0)
    claim("group_robbed", P_MANY, "main", M.add(320.0, 240.0, flip(tail, 218, 228)), 100, False)
    claim("group_steals", P_MANY, "main", M.add(321.0, 240.0, flip(tail, 225, 228)), 100)
    # the minimum stands twice, at list positions 5 and 64 + 3: the lower position wins, not the lower lane (run "high": the tie is accepted)
    claim("dup", P_MANY, "high", M.add(320.0, 241.0, 0), 5)
    KP["dup:later"] = 67

    # ---- the beyond-the-image bounds: a .5 position in x and one in y, found in the specification's arithmetic (run "beyond")
    Y1, Y2 = fr[BEY1], fr[BEY2]
    for axis, name in ((0, "beyond_half_x"), (1, "beyond_half_y")):
        found = [(k, half_position(BEYOND, axis, k)) for k in range(6, 40)]
        found = [(k, v) for k, v in found if v is not None]
        for j, under in enumerate((False, True)):
            k, v = found[0] if j == 0 else next(kv for kv in found if kv[0] >= found[0][0] + 5)
            other = F32(200.0 + 100 * j + 37 * axis)
            pa, pb, qc = [other, other], [other, other], [other, other]
            pa[axis], pb[axis], qc[axis] = nxt(v, -1e9) if under else v, F32(v - 3.0), F32(v - 1.0)
            a = Y2.add(pa[0], pa[1], 5)
            b = Y2.add(pb[0], pb[1], 5)
            nm = name + ("_under" if under else "")
            claim(nm, P_BEY, "beyond", Y1.add(qc[0], qc[1], 0), a if under else b)
            KP[nm + ":a"], KP[nm + ":b"], KP[nm + ":cell"] = a, b, k

    # ---- (l) the sizes: FULL has 256 keypoints, 65 of them level 0 inside the grid, in clusters of close descriptors (steals, ties, skips)
    rng = np.random.default_rng(648)
    Fu = fr[FULL]
    centres = rng.uniform((40, 40), (600, 440), (13, 2))
    bases = rng.integers(0, 256, (13, 32)).astype(np.uint8)
    for i in range(CAP):
        c = i % 13
        p = centres[c] + rng.normal(0, 4.0, 2)
        Fu.add(F32(p[0]), F32(p[1]), flip(bases[c], 0, int(rng.integers(0, 40))), octave=0 if i < 65 else int(rng.integers(1, 8)))
    for i in range(40):
        fr[NOLEVEL0].add(*site(i), 0, octave=1 + i % 7)
    fr[TWO].add(321.0, 240.0, 5); fr[TWO].add(319.0, 241.0, 30)
    claim("n0_one", P_ONE, "main", 0, 0)
    claim("n0_two", P_TWO, "main", 0, 0)
    fr[NEG].add(100.0, 100.0, 0); fr[OVER].add(100.0, 100.0, 0)

    counts = np.array([[f.n, 0] for f in fr], np.int32)
    counts[NEG, 0], counts[OVER, 0] = -1, CAP + 1
    kps, dsc = np.stack([f.kps for f in fr]), np.stack([f.desc for f in fr])
    prev = np.full((len(PAIRS), CAP, 2), -777.25, np.float32)
    for p, (ia, _) in enumerate(PAIRS.tolist()):
        n = int(np.clip(counts[ia, 0], 0, CAP)) if 0 <= ia < K else 0
        prev[p, :n, 0], prev[p, :n, 1] = kps[ia, :n]["x"], kps[ia, :n]["y"]
    for (p, q), c in moved.items():
        prev[p, q] = c
    assert counts[FULL, 0] == CAP and counts[EMPTY, 0] == 0 and counts[MANYQ, 0] > 64
    return dict(kps=kps, desc=dsc, counts=counts, pairs=PAIRS.copy(), prev=prev)


def frame(c, f):
    n = int(c["counts"][f, 0])
    return c["kps"][f, :n], c["desc"][f, :n]


def reference_view(k1):
    """F1's keypoints as the reference routine is to be given them.  The header counts a negative octave as "not level 0"; the reference
    tests `octave > 0` and then searches all levels, an input no extractor produces.  The one planted query of that kind (oct_qneg) goes to
    the reference with octave 1, which the header declares equivalent."""
    k = k1.copy()
    k["octave"][k["octave"] < 0] = 1
    return k


PLANTED, KP, CLAIMS = {}, {}, {}
