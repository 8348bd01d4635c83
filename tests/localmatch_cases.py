"""One constructed batch for the batched SearchLocalPoints (include/orbx_localmatch.h): 13 items over 5 frames, capacity 256, 320 points a
local map, 8 levels.  Every edge of the specification is planted at a site of its own in frame PLANT (sites are 70 pixels apart: no window
of one reaches another at th = 1), the statistical conditions come from the derived items.  PLANTED names the points, KP the keypoints.
numpy only: the CPU test holds the batch to its claims on tests/localmatch_model.py, the GPU test runs it."""
import numpy as np

from orb_slam3_modified_amd._lib import KP_DTYPE
from orb_slam3_modified_amd.localmatch import POINT_DTYPE

F32 = np.float32
K, CAP, MCAP, NLEVELS = 5, 256, 320, 8
RANDOM, PLANT, EMPTY, FULL, BADCOUNT = 0, 1, 2, 3, 4          # the frames
NN_RATIO = 0.8
TH = (1.0, 3.0)
BOUNDS = np.array([[0, 0, 640, 480], [0, 0, 640, 480], [0, 0, 640, 480], [-12.5, -7.25, 655.0, 490.5], [0, 0, 640, 480]], np.float32)
# the items: 0 derived (with doubled points), 1 the planted sites, 2 the dense cluster, 3 an empty frame, 4 nmp = 0, 5 nothing in view,
# 6 a full frame with nmp = mcap, 7 frame RANDOM again with another kp_obs row; 8 .. 12 malformed, one of each kind
I_DERIVED, I_PLANT, I_DENSE, I_EMPTY, I_NOPOINTS, I_NOVIEW, I_FULL, I_AGAIN = range(8)
MALFORMED = {8: "frame", 9: "count", 10: "nmp", 11: "level", 12: "point"}
B = 13
SMALL_ROOM = 128                                                # candidates beyond one longest list that the lowered LDS limit of the GPU test leaves
VC_EDGE = F32(0.998)                                            # above the double literal 0.998: radius 2.5
VC_BELOW = np.nextafter(F32(0.998), F32(0))                     # below it: radius 4.0


def scale_factors():
    s = np.ones(NLEVELS, np.float32)
    for i in range(1, NLEVELS):
        s[i] = F32(s[i - 1] * F32(1.2))
    return s


def flip(desc, d):
    """desc with its first d bits flipped: Hamming distance d."""
    bits = np.unpackbits(desc)
    bits[:d] ^= 1
    return np.packbits(bits)


class _Frame:
    def __init__(self):
        self.kps, self.desc, self.ur = np.zeros(CAP, KP_DTYPE), np.zeros((CAP, 32), np.uint8), np.full(CAP, -1.0, np.float32)
        self.n = 0

    def add(self, x, y, octave, desc, ur=-1.0):
        i = self.n
        self.kps[i]["x"], self.kps[i]["y"], self.kps[i]["octave"], self.kps[i]["size"] = x, y, octave, 31.0
        self.desc[i], self.ur[i] = desc, ur
        self.n += 1
        return i


class _Item:
    def __init__(self, frame, pool):
        self.frame, self.pool, self.mp, self.n = frame, pool, np.zeros(MCAP, POINT_DTYPE), 0

    def add(self, x, y, level, desc, obs=1, vc=0.9, xr=0.0, in_view=1):
        q = self.n
        self.pool.append(np.asarray(desc, np.uint8))
        self.mp[q] = (x, y, xr, vc, level, obs, len(self.pool) - 1, in_view)
        self.n += 1
        return q


def _derived(rng, item, fr, count, doubled):
    """Points in the style of tests/test_gpu_search.py::_map_points: keypoints of the frame seen as map points, with drift and noise; the
    first `doubled` of them twice, the first copy with obs > 0: the second cannot have the keypoint."""
    src = rng.permutation(fr.n)[:count]
    src = np.concatenate([src, src[:doubled]])
    first = np.zeros(len(src), bool)
    first[:doubled] = True
    order = np.argsort(np.concatenate([np.arange(count) * 2, np.arange(doubled) * 2 + 1]), kind="stable")   # a copy right after its original
    for j in order:
        i = int(src[j])
        kp = fr.kps[i]
        x, y = F32(kp["x"] + 1.0 + rng.normal(0, 0.6)), F32(kp["y"] + 0.5 + rng.normal(0, 0.6))
        d = fr.desc[i].copy()
        d[rng.integers(0, 32, 3)] ^= rng.integers(0, 256, 3).astype(np.uint8)
        disp = kp["x"] - fr.ur[i] if fr.ur[i] > 0 else 9.0
        item.add(x, y, int(np.clip(kp["octave"] + rng.integers(0, 2), 0, NLEVELS - 1)), d, obs=int(rng.choice([1, 3, 7])) if first[j] else int(rng.choice([0, 0, 1, 3, 7])),
                 vc=rng.choice([0.9, 0.9979, 0.998, 0.9981, 1.0]), xr=F32(x - disp + rng.normal(0, 0.5)), in_view=int(rng.random() < 0.9) if not first[j] else 1)


def build():
    """-> dict(kps [K, CAP], desc, counts [K, 2], uright [K, CAP], bounds [K, 4], frames [B], mp [B, MCAP], nmp [B], pdesc [M, 32], kp_obs [B, CAP],
    sf [NLEVELS]) and fills PLANTED / KP."""
    rng = np.random.default_rng(1904)
    rd = lambda: rng.integers(0, 256, 32).astype(np.uint8)   # noqa: E731
    fr = [_Frame() for _ in range(K)]
    pool = []
    # ---- frames RANDOM and FULL: clustered keypoints (windows with several candidates), half of them stereo
    for f, n in ((RANDOM, 200), (FULL, CAP)):
        lo, hi = BOUNDS[f, :2], BOUNDS[f, 2:]
        centres = rng.uniform(lo + 20, hi - 20, (n // 4, 2))
        for i in range(n):
            c = centres[i % len(centres)] + rng.normal(0, 3.0, 2)
            x = F32(c[0])
            fr[f].add(x, F32(c[1]), int(rng.choice([0, 0, 1, 1, 2, 3, 5, 7])), rd(), F32(x - rng.uniform(2, 30)) if rng.random() < 0.5 else -1.0)
    fr[FULL].kps[5]["x"], fr[FULL].kps[6]["y"] = -40.0, 900.0   # two features in no cell
    fr[BADCOUNT].add(100.0, 100.0, 0, rd())
    P = fr[PLANT]
    items = [_Item(f, pool) for f in (RANDOM, PLANT, PLANT, EMPTY, RANDOM, RANDOM, FULL, RANDOM, K, BADCOUNT, RANDOM, RANDOM, RANDOM)]
    it = items[I_PLANT]
    obs_in = {}                                                   # planted kp_obs values of item I_PLANT
    site = lambda s: (F32(60 + 70 * (s % 8)), F32(60 + 70 * (s // 8)))   # noqa: E731
    PLANTED.clear(); KP.clear()

    # (a) view_cos at float32(0.998): radius 2.5 misses a keypoint 3 pixels away; one ulp below: radius 4.0 takes it
    for s, name, vc in ((0, "cos_edge", VC_EDGE), (1, "cos_below", VC_BELOW)):
        x, y = site(s)
        d = rd()
        KP[name] = P.add(x + 3.0, y, 0, flip(d, 2))
        PLANTED[name] = it.add(x, y, 0, d, vc=vc)
    # (b) th: 6 pixels away at level 0 is outside 4.0 and inside 4.0 * 3.0
    x, y = site(2)
    d = rd()
    KP["th"] = P.add(x, y + 6.0, 0, flip(d, 1))
    PLANTED["th"] = it.add(x, y, 0, d)
    # (c) level 0 takes octave 0 (and not the better octave 1); level 7 takes octaves 6 and 7 (and not the better octave 5)
    x, y = site(3)
    d = rd()
    KP["lvl0"], _ = P.add(x + 1.0, y, 0, flip(d, 20)), P.add(x - 1.0, y, 1, flip(d, 0))
    PLANTED["lvl0"] = it.add(x, y, 0, d)
    x, y = site(4)
    d = rd()
    P.add(x + 1.0, y, 5, flip(d, 0))
    KP["lvl7"] = P.add(x - 2.0, y + 1.0, 6, flip(d, 25))
    P.add(x, y - 2.0, 7, flip(d, 90))
    PLANTED["lvl7"] = it.add(x, y, NLEVELS - 1, d)
    # (e) best and second on one octave at the ratio boundary: float32(0.8) * 50 rounds to 40.0, so 40 stays and 41 goes; with the second on
    # another octave 41 stays
    for s, name, best, octave2 in ((5, "ratio_at", 40, 2), (6, "ratio_over", 41, 2), (7, "ratio_other_octave", 41, 1)):
        x, y = site(s)
        d = rd()
        KP[name] = P.add(x + 1.0, y, 2, flip(d, best))
        P.add(x - 1.0, y, octave2, flip(d, 50))
        PLANTED[name] = it.add(x, y, 2, d)
    # (f) two points want one keypoint, the first has obs > 0: the second takes the runner-up ...
    x, y = site(8)
    d = rd()
    KP["taken"], KP["runner_up"] = P.add(x, y + 1.0, 1, d), P.add(x + 1.0, y, 0, flip(d, 30))
    PLANTED["first"], PLANTED["second_runner_up"] = it.add(x, y, 1, d, obs=3), it.add(x, y, 1, d, obs=2)
    # ... or fails the ratio among the survivors (30 > 0.8 * 32) where the first passed it (0 <= 0.8 * 30)
    x, y = site(9)
    d = rd()
    KP["taken2"] = P.add(x, y + 1.0, 1, d)
    P.add(x + 1.0, y, 1, flip(d, 30)); P.add(x - 1.0, y, 1, flip(d, 32))
    PLANTED["first2"], PLANTED["second_fails"] = it.add(x, y, 1, d, obs=1), it.add(x, y, 1, d, obs=1)
    # (g) the same pair with obs = 0: the keypoint is rebound, both count
    x, y = site(10)
    d = rd()
    KP["rebound"] = P.add(x, y + 1.0, 1, d)
    P.add(x + 1.0, y, 0, flip(d, 30))
    PLANTED["unobserved"], PLANTED["rebinds"] = it.add(x, y, 1, d, obs=0), it.add(x, y, 1, d, obs=5)
    # (h) kp_obs arriving as -1, 0 and positive: only the positive one hides its keypoint
    for s, name, v in ((11, "obs_none", -1), (12, "obs_zero", 0), (13, "obs_positive", 4)):
        x, y = site(s)
        d = rd()
        KP[name] = P.add(x + 1.0, y, 0, flip(d, 3))
        obs_in[KP[name]] = v
        PLANTED[name] = it.add(x, y, 0, d)
    # (i) the stereo gate at er == radius (kept), one ulp above (dropped on a stereo side), and u_right zero and negative (no gate)
    for s, name, ur, er in ((14, "gate_at", 1.0, F32(4.0)), (15, "gate_over", 1.0, np.nextafter(F32(4.0), F32(5.0))), (16, "gate_zero", 0.0, 50.0),
                            (17, "gate_negative", -1.0, 50.0)):
        x, y = site(s)
        d = rd()
        KP[name] = P.add(x + 1.0, y, 0, flip(d, 3), ur)
        PLANTED[name] = it.add(x, y, 0, d, xr=F32(F32(ur) + F32(er)))
    # the four early returns of GetFeaturesInArea, a non-finite projection, an out-of-view point with a level and a row that are none
    for name, x, y in (("return_min_x", 700.0, 100.0), ("return_max_x", -60.0, 100.0), ("return_min_y", 100.0, 540.0), ("return_max_y", 100.0, -60.0),
                       ("nan", np.nan, 100.0), ("inf", 100.0, np.inf)):
        PLANTED[name] = it.add(x, y, 0, rd())
    PLANTED["nan_cos"] = it.add(*site(0), 0, rd(), vc=np.nan)
    PLANTED["out_of_view"] = it.add(*site(0), 99, rd(), in_view=0)
    it.mp[PLANTED["out_of_view"]]["point"] = 2 ** 30

    # (d) item I_DENSE: 72 keypoints of octaves 6 and 7 around site 20, twelve level-7 points over them (more than 64 surviving candidates a
    # point: two chain trips; more candidates in the item than a lowered LDS limit leaves room for: several chunks).  The minimum stands
    # twice, in grid columns 19 and 21: the walk meets column 19 first although its keypoint has the larger index
    cx, cy = F32(200.0), F32(270.0)
    dd = rd()
    KP["dup_later_column"] = P.add(cx + 9.0, cy, 7, dd)          # column round(20.9) = 21
    for j in range(70):
        P.add(F32(cx - 8.0 + 2.0 * (j % 9)), F32(cy - 8.0 + 2.0 * (j // 9)), 6 + j % 2, flip(rd(), j))
    KP["dup_first_column"] = P.add(cx - 9.0, cy, 7, dd)          # column round(19.1) = 19
    dn = items[I_DENSE]
    PLANTED["dup"] = dn.add(cx, cy, NLEVELS - 1, dd, obs=0)
    for j in range(11):
        dn.add(F32(cx - 3.0 + j * 0.5), F32(cy + 1.0), NLEVELS - 1, P.desc[KP["dup_later_column"] + 1 + 6 * j], obs=j % 3)

    # ---- the derived items
    _derived(rng, items[I_DERIVED], fr[RANDOM], 175, 60)          # 235 points: no multiple of 64
    for q in range(10):
        items[I_EMPTY].add(F32(100 + 30 * q), 200.0, 0, rd())
    for q in range(64):
        items[I_NOVIEW].add(F32(100 + 5 * q), 200.0, -7, rd(), in_view=0)
    _derived(rng, items[I_FULL], fr[FULL], 250, 70)               # 320 = MCAP points
    _derived(rng, items[I_AGAIN], fr[RANDOM], 150, 0)
    # ---- the malformed items: each is item I_AGAIN's row with one value out of range
    for b, kind in MALFORMED.items():
        items[b].mp[:], items[b].n = items[I_AGAIN].mp, items[I_AGAIN].n
    live = np.nonzero(items[11].mp[:items[11].n]["in_view"])[0]
    items[11].mp[live[-1]]["level"] = NLEVELS
    items[12].mp[live[0]]["point"] = len(pool)                     # the first row past the pool

    assert it.n <= MCAP and P.n <= CAP and items[I_FULL].n == MCAP and items[I_DERIVED].n % 64
    c = dict(kps=np.stack([f.kps for f in fr]), desc=np.stack([f.desc for f in fr]), uright=np.stack([f.ur for f in fr]), bounds=BOUNDS.copy(),
             counts=np.array([[f.n, 0] for f in fr], np.int32), frames=np.array([i.frame for i in items], np.int32),
             mp=np.stack([i.mp for i in items]), nmp=np.array([i.n for i in items], np.int32), pdesc=np.stack(pool), sf=scale_factors())
    c["counts"][BADCOUNT, 0] = CAP + 1
    c["nmp"][10] = MCAP + 1
    kp_obs = rng.choice([-1, -1, -1, 0, 2], (B, CAP)).astype(np.int32)
    kp_obs[I_PLANT] = -1
    for i, v in obs_in.items():
        kp_obs[I_PLANT, i] = v
    kp_obs[I_DENSE] = -1
    c["kp_obs"] = kp_obs
    assert c["mp"].shape == (B, MCAP) and c["counts"][EMPTY, 0] == 0 and c["counts"][FULL, 0] == CAP
    return c


PLANTED, KP = {}, {}
