"""The constructed batch of the Sim3 projection-front tests (CPU model test and GPU test share it): 8 items, mcap 96 (one full wave and half
of the next), 8 levels at scale factor 1.2.  proj and fuse read tests/project_cases.py's batch as it stands: the same pose items, the same
point lists (as indices) and its table, so every edge planted there for Fuse's gates (z = -0.0f, +0.0f and negative, each bound and the
float outside it, a NaN position, dist on min_inv / max_inv, dot == 0.5 * dist, the ratios on the thresholds of both log kinds, dist = 0)
is planted here.  search reads the same lists over that table with a few points appended, through items of its own:
  items 0 .. 2  as there: nslots = 0, an index equal to npoints, nslots = mcap + 1
  item 3, 6     pose A, then the similarity SA (s = 1.07, about 0.05 rad): a scale that is no power of two
  item 4        the identity pose and the identity similarity (s = 1, t = -0.0, q = (0, 0, 0, 1)): under the matrix forms Pb = P exactly,
                so the planted points of tests/project_cases.py are planted in the target's camera frame too
  item 5        pose B, then the similarity SB (s = 0.83, about 0.4 rad)
  item 7        the identity pose and the similarity (s = 2, R = I, t = -0.0): Pb = 2 P exactly, the projection stays and dist3D doubles
The appended points are found by search on the model under the identity item: operands for which fx * x + cx fused differs from the product
and the sum, for which Pb[0] * invz differs from Pb[0] / Pb[2], and for which Pinhole::project's (fx * X) / Z + cx (:427) differs from
fx * (X * invz) + cx (:534, SearchBySim3).  agree_block() is the planted block of the agreement pass,
chain_world() the two-keyframe side of the chain tests."""
import functools
from fractions import Fraction

import numpy as np

from tests import project_cases as pc
from tests import sim3_model as sm
from tests.project_cases import MCAP, NITEMS, NLEVELS, SCALE_FACTOR, THRESHOLD_LEVELS, pose  # noqa: F401
from tests.sim3_model import F, FUSE, PROJ, PROJ_KFS, SEARCH

KINDS = (PROJ, FUSE, SEARCH, PROJ_KFS)   # PROJ_KFS: proj under PROJ_INVZ, the vpPointsKFs overload
NEXTRA = 3                          # the points appended to tests/project_cases.py's table
NPOINTS = pc.NPOINTS + NEXTRA
IDENT = 4                           # the item over the planted points
OPTIONS = [(r, s, k) for r in (sm.ROT_MATRIX, sm.ROT_QUAT) for s in (sm.SUM_LTR, sm.SUM_TREE) for k in (sm.LOG_DOUBLE, sm.LOG_FLOAT)]
SIM_KINDS = (sm.SIM3_MATRIX, sm.SIM3_QUAT)


def similarity(s, axis, angle, t):
    """(s, R, t, q) in float32 from float64: R the unit rotation, q the RxSO3's quaternion (x, y, z, w) of squared norm s."""
    R, t, _, q = pose(axis, angle, t)
    return F(s), R, t, (q.astype(np.float64) * np.sqrt(s)).astype(F)


def inverse(S):
    """S^-1 from float64: (1 / s, R^T, -(R^T t) / s)."""
    s, R, t, q = S
    R64 = R.reshape(3, 3).astype(np.float64)
    qi = np.array([-q[0], -q[1], -q[2], q[3]], np.float64) / float(s)       # conj / |q|^2 has squared norm 1 / s
    return F(1.0 / float(s)), R64.T.astype(F).ravel(), (-(R64.T @ t.astype(np.float64)) / float(s)).astype(F), qi.astype(F)


def sim3_item(T, S, fx, fy, cx, cy, bounds, th):
    """A record of ITEM_DTYPE from a pose (Rcw, tcw, Ow, q) and a similarity (s, R, t, q)."""
    it = np.zeros((), sm.ITEM_DTYPE)
    it["Raw"], it["taw"], it["qa"] = T[0], T[1], T[3]
    it["s"], it["Rba"], it["tba"], it["qba"] = S
    it["fx"], it["fy"], it["cx"], it["cy"], it["bounds"], it["th"] = fx, fy, cx, cy, bounds, th
    return it


def _of_pose_item(p, S):
    return sim3_item((p["Rcw"], p["tcw"], p["Ow"], p["q"]), S, p["fx"], p["fy"], p["cx"], p["cy"], p["bounds"], p["th"])


IDENTITY = (F(1), np.eye(3, dtype=F).ravel(), F(-0.0) * np.ones(3, F), np.array([0, 0, 0, 1], F))
DOUBLE = (F(2), np.eye(3, dtype=F).ravel(), F(-0.0) * np.ones(3, F), np.array([0, 0, 0, np.sqrt(2.0)], F))


@functools.lru_cache(maxsize=None)
def batch():
    """dict(points, items (pose items), sitems (search items), idx, nslots, lsf, sf, planted): planted maps a case's name to (slot of item
    4, {kind: exit})."""
    b = pc.batch()
    rng = np.random.RandomState(2626)
    points = np.zeros(NPOINTS, sm.TABLE_DTYPE)
    points[:pc.NPOINTS] = b["points"]
    SA = similarity(1.07, (0.3, -0.2, 1.0), 0.05, (0.02, -0.03, 0.05))
    SB = similarity(0.83, (1.0, 0.1, -0.4), 0.4, (-0.1, 0.05, 0.2))
    sitems = np.zeros(NITEMS, sm.ITEM_DTYPE)
    for i, S in enumerate((SA, SA, SA, SA, IDENTITY, SB, SA, DOUBLE)):
        sitems[i] = _of_pose_item(b["items"][i], S)
    ident = sitems[IDENT]

    def trace(P):
        tab = np.zeros(1, sm.TABLE_DTYPE)
        tab[0] = (np.array(P, F), 0, (0, 0, 1), np.inf, 1, (0, 0, 0))
        return sm.project_slot(SEARCH, ident, tab, 0, b["lsf"], NLEVELS, b["sf"])

    # tests/project_cases.py's planted cases, with the exit each emitter takes: proj's and fuse's gates are Fuse's of §25; search has no
    # viewing-angle gate
    fuse_exit = lambda e: {PROJ: e[pc.FUSE], PROJ_KFS: e[pc.FUSE], FUSE: e[pc.FUSE],   # noqa: E731
                           SEARCH: sm.VALID if e[pc.FUSE] == sm.ANGLE else e[pc.FUSE]}
    assert (sm.DEPTH, sm.U, sm.V, sm.DISTANCE, sm.ANGLE, sm.VALID) == (pc.pm.DEPTH, pc.pm.U, pc.pm.V, pc.pm.DISTANCE, pc.pm.ANGLE, pc.pm.VALID)
    planted = {name: (slot, fuse_exit(exits)) for name, (slot, exits) in b["planted"].items()}
    # the appended points
    need = {"u_not_fused": None, "x_multiplies": None, "overloads_differ": None}
    pose_ident = b["items"][IDENT]
    while any(v is None for v in need.values()):
        P = np.array([rng.rand() * 2 - 1, rng.rand() - 0.5, 1 + rng.rand() * 3], F)
        row, why, tr = trace(P)
        if why != sm.VALID:
            continue
        fused = F(float(Fraction(float(ident["fx"])) * Fraction(float(tr["x"])) + Fraction(float(ident["cx"]))))
        if need["u_not_fused"] is None and fused != row[0]:
            need["u_not_fused"] = P
        elif need["x_multiplies"] is None and ident["fx"] * (P[0] / P[2]) + ident["cx"] != row[0]:
            need["x_multiplies"] = P
        elif need["overloads_differ"] is None and (pose_ident["fx"] * P[0]) / P[2] + pose_ident["cx"] != row[0]:
            need["overloads_differ"] = P                         # :427's Pinhole::project against :534's invz form, in u
    idx = b["idx"].copy()
    tail = [MCAP - 1 - n for n in range(NEXTRA)]                  # the identity item's list ends in points that random slots list too
    assert all(idx[IDENT, j] < pc.NRANDOM for j in tail)
    for n, (name, P) in enumerate(need.items()):
        d = F(np.sqrt((P[0] * P[0] + P[1] * P[1]) + P[2] * P[2]))
        points[pc.NPOINTS + n] = (P, 0, P / d, np.inf, d, (0, 0, 0))
        idx[IDENT, tail[n]] = pc.NPOINTS + n
        planted[name] = (tail[n], {PROJ: sm.VALID, PROJ_KFS: sm.VALID, FUSE: sm.VALID, SEARCH: sm.VALID})
    idx[7] = idx[IDENT][::-1]
    idx[1, 57] = NPOINTS                                          # item 1 stays malformed: one past THIS table
    for a_ in (points, sitems, idx):
        a_.setflags(write=False)                                  # shared among the tests: left unchanged
    return dict(points=points, items=b["items"], sitems=sitems, idx=idx, nslots=b["nslots"], lsf=b["lsf"], sf=b["sf"], planted=planted)


@functools.lru_cache(maxsize=None)
def expected(kind: int, rot_kind: int, sum_order: int, log_kind: int, sim_kind: int = sm.SIM3_MATRIX):
    """The model's (rows, nvalid, exits) for the batch, computed once per emitter and option tuple (proj and fuse do not read sim_kind)."""
    if kind != SEARCH and sim_kind != sm.SIM3_MATRIX:
        return expected(kind, rot_kind, sum_order, log_kind)
    b = batch()
    return sm.project(kind, b["points"], b["sitems"] if kind == SEARCH else b["items"], b["idx"], b["nslots"], b["lsf"], NLEVELS,
                      None if kind in (PROJ, PROJ_KFS) else b["sf"], log_kind, rot_kind, sum_order, sim_kind)


# ------------------------------------------------------------------------------------------------------------------- the agreement pass
AGREE_QCAP = 70                     # one wave and six lanes


@functools.lru_cache(maxsize=None)
def agree_block():
    """The planted block of the agreement pass: dict(idx12, dist12, nf12, idx21, dist21, nf21, n1, n2) for 7 pairs.
      pair 0  random rows with a planted prefix: i1 = 0 and 1 both choose idx2 = 3, whose vnMatch2 names 1; best_dist exactly 100 (kept) and
              101 (dropped) on either side; idx2 equal to n2, beyond it and beyond qcap; a negative idx2
      pair 1  n1 = 0;  pair 2  n2 = 0
      pair 3  input nfound12 = -1;  pair 4  input nfound21 = -1
      pair 5  n1 = qcap + 1;  pair 6  n2 = -1"""
    rng = np.random.RandomState(99)
    P, Q = 7, AGREE_QCAP
    n1 = np.array([66, 0, 50, 40, 40, Q + 1, 30], np.int32)
    n2 = np.array([59, 40, 0, 40, 40, 30, -1], np.int32)
    idx12, idx21 = rng.randint(-1, 64, (P, Q)).astype(np.int32), rng.randint(-1, 64, (P, Q)).astype(np.int32)
    dist12, dist21 = rng.randint(0, 140, (P, Q)).astype(np.int32), rng.randint(0, 140, (P, Q)).astype(np.int32)
    # mutual partners among the random rows of pair 0: i1 <-> 63 - i1 for a third of the row
    for i1 in range(10, 60, 3):
        idx12[0, i1], idx21[0, 63 - i1] = 63 - i1, i1
        dist12[0, i1], dist21[0, 63 - i1] = rng.randint(0, 101), rng.randint(0, 101)
    idx12[0, :10] = (3, 3, 5, 6, 7, 59, 60, 10 ** 6, -1, 8)
    dist12[0, :10] = (10, 20, 100, 101, 30, 5, 5, 5, 5, 40)
    idx21[0, 3], dist21[0, 3] = 1, 50                             # vnMatch2[3] names i1 = 1: i1 = 0 loses
    idx21[0, 5], dist21[0, 5] = 2, 100                            # 100 on both sides: kept
    idx21[0, 6], dist21[0, 6] = 3, 10                             # its partner's best_dist is 101: dropped
    idx21[0, 7], dist21[0, 7] = 4, 101                            # 101 on the other side: dropped
    idx21[0, 8], dist21[0, 8] = 9, 0                              # a plain mutual pair
    nf12, nf21 = np.array([9, 0, 4, -1, 3, 2, 2], np.int32), np.array([7, 1, 0, 5, -1, 2, 2], np.int32)
    out = dict(idx12=idx12, dist12=dist12, nf12=nf12, idx21=idx21, dist21=dist21, nf21=nf21, n1=n1, n2=n2)
    for a_ in out.values():
        a_.setflags(write=False)
    return out


def agree_args(b):
    return b["idx12"], b["dist12"], b["nf12"], b["idx21"], b["dist21"], b["nf21"], b["n1"], b["n2"]


# ---------------------------------------------------------------------------------------------------------------- the chain tests' side
def pose_chain_world():
    """tests/project_cases.py's two-keyframe chain world, with matcher items of the Sim3 kind: (3, 1.5), LoopClosing's first call."""
    from orb_slam3_modified_amd import projmatch
    w = dict(pc.chain_world())
    w["sim3_items"] = np.array([(f, projmatch.KIND_SIM3, 3.0, projmatch.max_dist_sim3(1.5)) for f in w["pairs"]], projmatch.ITEM_DTYPE)
    return w


@functools.lru_cache(maxsize=None)
def chain_world():
    """A SearchBySim3 batch of two pairs over a side of two keyframes, both tests/lastmatch_cases.py's frame RANDOM (about 200 keypoints),
    each with a pose of its own.  About half of each keyframe's keypoints hold a map point of the keyframe's own (table rows [0, N) and
    [N, 2 N)), lifted through the keyframe's pose at one of four depths; its descriptor is the keypoint's with one bit flipped and its
    max_dist makes the predicted level the keypoint's octave.  The similarity between the two cameras is near the identity, so a point of
    keypoint j lands near keypoint j of the other keyframe: most keypoints that hold a point in both keyframes agree.  Pair 0 is
    (keyframe 0, keyframe 1) with S12 = SC, pair 1 is (keyframe 1, keyframe 0) with another similarity; slot j is keypoint j."""
    from orb_slam3_modified_amd import fuse
    from tests import frustum_model as fm
    from tests import lastmatch_cases as lc
    c = lc.build()
    frames = [lc.RANDOM, lc.RANDOM]
    rng = np.random.RandomState(78)
    sf = c["sf"]
    n, cap = int(c["counts"][lc.RANDOM, 0]), lc.CAP
    kp, bounds = c["kps"][lc.RANDOM, :n], c["bounds"][lc.RANDOM]
    fx, fy = 435.2, 436.1
    cx, cy = F(0.5 * (bounds[0] + bounds[2]) + 1.215), F(0.5 * (bounds[1] + bounds[3]) - 0.625)
    T = [pose((0.3, 1.0, 0.2), 0.05, (0.0, -0.05, 0.2)), pose((0.1, -1.0, 0.3), 0.4, (0.3, 0.1, -0.2))]
    table, pdesc = np.zeros(2 * n, sm.TABLE_DTYPE), np.zeros((2 * n, 32), np.uint8)
    idx = np.full((2, cap), -1, np.int32)                         # per keyframe: the map point of each keypoint
    for f in range(2):
        R64, t64 = T[f][0].reshape(3, 3).astype(np.float64), T[f][1].astype(np.float64)
        z = np.array([1.5, 2.5, 4.0, 6.0])[(np.arange(n) + f) % 4]
        Pc = np.stack([(kp["x"] - cx) * z / fx, (kp["y"] - cy) * z / fy, z], 1)
        P = ((Pc - t64) @ R64).astype(F)                          # R^T (Pc - t)
        dist = np.linalg.norm(Pc, axis=1)                         # the camera-frame norm: what dist3D is, up to the similarity
        maxd = (dist * 1.2 ** kp["octave"] * 0.95).astype(F)
        rows = slice(f * n, (f + 1) * n)
        table["pos"][rows], table["normal"][rows] = P, (0, 0, 1)  # the normal is not read
        table["min_inv"][rows], table["max_inv"][rows], table["max_dist"][rows] = F(0.8) * (maxd / F(4.3)), F(1.2) * maxd, maxd
        desc = c["desc"][lc.RANDOM, :n].copy()
        desc[np.arange(n), rng.randint(0, 32, n)] ^= np.uint8(1) << rng.randint(0, 8, n).astype(np.uint8)
        pdesc[rows] = desc
        holds = rng.rand(n) < 0.7                                 # no map point, a bad one or one already matched elsewhere
        idx[f, :n] = np.where(holds, f * n + np.arange(n), -1 - (np.arange(n) % 3))
    SC = similarity(1.02, (0.5, 0.2, 1.0), 0.004, (0.004, -0.003, 0.01))
    SD = similarity(0.97, (-0.2, 1.0, 0.1), 0.003, (-0.005, 0.002, -0.02))
    # pair p: keyframe 1 = kf1[p], keyframe 2 = kf2[p]; items12 = (T_1w, S21, bounds of 2), items21 = (T_2w, S12, bounds of 1)
    kf1, kf2 = np.array([0, 1], np.int32), np.array([1, 0], np.int32)
    items12, items21 = np.zeros(2, sm.ITEM_DTYPE), np.zeros(2, sm.ITEM_DTYPE)
    for p, S12 in enumerate((SC, SD)):
        items12[p] = sim3_item(T[kf1[p]], inverse(S12), fx, fy, cx, cy, bounds, 7.5)
        items21[p] = sim3_item(T[kf2[p]], S12, fx, fy, cx, cy, bounds, 7.5)
    counts = np.ascontiguousarray(c["counts"][frames])
    side = dict(kps=np.ascontiguousarray(c["kps"][frames]), desc=np.ascontiguousarray(c["desc"][frames]), counts=counts,
                uright=np.ascontiguousarray(c["uright"][frames]), bounds=np.ascontiguousarray(c["bounds"][frames]), nframes=2, capacity=cap)
    side["gridparm"] = np.stack([fuse.grid_parameters(*b_) for b_ in side["bounds"]])
    n1, n2 = np.ascontiguousarray(counts[kf1, 0]), np.ascontiguousarray(counts[kf2, 0])
    return dict(table=table, pdesc=pdesc, items12=items12, items21=items21, idx1=np.ascontiguousarray(idx[kf1]), idx2=np.ascontiguousarray(idx[kf2]),
                n1=n1, n2=n2, kf1=kf1, kf2=kf2, sf=sf, lsf=fm.log_scale_factor(SCALE_FACTOR), side=side)


@functools.lru_cache(maxsize=None)
def chain_expected():
    """The model chain on chain_world(): sim3_model's queries of both directions through tests/fuse_model.py (the gate off, th_low =
    TH_HIGH) and sim3_model.agree -> dict(q12, q21 (rows, nvalid), r12, r21 (nfound, best_idx, best_dist), match12, nfound)."""
    from tests import fuse_model
    w = chain_world()
    s = w["side"]
    q12 = sm.project(SEARCH, w["table"], w["items12"], w["idx1"], w["n1"], w["lsf"], scale_factors=w["sf"])[:2]
    q21 = sm.project(SEARCH, w["table"], w["items21"], w["idx2"], w["n2"], w["lsf"], scale_factors=w["sf"])[:2]
    r12 = fuse_model.search(s["kps"], s["desc"], s["counts"], s["uright"], s["gridparm"], q12[0], w["n1"], w["kf2"], w["pdesc"], None, False, 100)
    r21 = fuse_model.search(s["kps"], s["desc"], s["counts"], s["uright"], s["gridparm"], q21[0], w["n2"], w["kf1"], w["pdesc"], None, False, 100)
    match12, nfound = sm.agree(r12[1], r12[2], r12[0], r21[1], r21[2], r21[0], w["n1"], w["n2"], 100)
    return dict(q12=q12, q21=q21, r12=r12, r21=r21, match12=match12, nfound=nfound)
