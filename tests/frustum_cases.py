"""The constructed batch of the frustum tests (CPU model test and GPU test share it): 4 items, mcap 130 (two full waves and a 2-lane tail of a
256-lane workgroup's first 192 lanes), a table of 200 points, 8 levels at scale factor 1.2.
  item 0  nmp = 0; its row holds indices no table has (never read)
  item 1  malformed: one index equal to npoints
  item 2  a pose a little off the identity over the random part of the table, far_th between two accepted depths, nmp = 129
  item 3  the identity pose (tcw = -0.0) over the planted points: with it Pc = P and PO = P exactly, so a point is planted by writing the
          camera coordinates the case needs; its list repeats indices and holds negative ones
Every planted case asserts here, on the CPU model, that the model takes the branch it was built for."""
import functools
import math
from fractions import Fraction

import numpy as np

from tests import frustum_model as fm
from tests.frustum_model import F

NITEMS, MCAP, NPOINTS, NLEVELS, SCALE_FACTOR, COS_LIMIT = 4, 130, 200, 8, 1.2, 0.5
NRANDOM = 110                       # table rows [0, NRANDOM) are random, the planted ones follow
OPTION_PAIRS = [(s, k) for s in (fm.SUM_LTR, fm.SUM_TREE) for k in (fm.LOG_DOUBLE, fm.LOG_FLOAT)]


def up(x):
    return np.nextafter(F(x), F(np.inf))


def down(x):
    return np.nextafter(F(x), F(-np.inf))


def _key(x) -> int:
    """An integer that orders floats as their values do."""
    u = int(np.array(x, F).view(np.uint32))
    return -(u & 0x7FFFFFFF) if u >> 31 else u


def _unkey(k: int):
    return np.array(k if k >= 0 else (-k) | 0x80000000, np.uint32).view(F)[()]


def solve(f, target, lo, hi):
    """x in [lo, hi] with f(x) == target for a non-decreasing float function f, by bisection over the floats."""
    a, b = _key(lo), _key(hi)
    while a < b:
        m = (a + b) // 2
        if f(_unkey(m)) < target:
            a = m + 1
        else:
            b = m
    x = _unkey(a)
    assert f(x) == target, (x, f(x), target)
    return x


def threshold(lsf, n: int, log_kind: int):
    """The largest float whose level is <= n, from the direct expression (bisection; the step is checked by test_frustum_model)."""
    lo, hi = 1, 0x7F7FFFFF
    while hi - lo > 1:
        m = (lo + hi) // 2
        if fm.level(np.array(m, np.uint32).view(F)[()], lsf, NLEVELS, log_kind) <= n:
            lo = m
        else:
            hi = m
    return np.array(lo, np.uint32).view(F)[()]


@functools.lru_cache(maxsize=None)
def batch():
    """dict(points, obs, items, idx, nmp, lsf, planted): planted maps a case's name to (item, slot, the exit it must take)."""
    rng = np.random.RandomState(2121)
    lsf = fm.log_scale_factor(SCALE_FACTOR)
    points, obs = np.zeros(NPOINTS, fm.TABLE_DTYPE), np.ones(NPOINTS, np.int32)
    items = np.zeros(NITEMS, fm.ITEM_DTYPE)
    idx, nmp = np.zeros((NITEMS, MCAP), np.int32), np.zeros(NITEMS, np.int32)

    # ---- the poses.  Items 0 .. 2: a rotation about y and one about x, Ow = -R^T t in the stand-ins' arithmetic
    a, c = F(0.05), F(-0.03)
    Ry = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]], F)
    Rx = np.array([[1, 0, 0], [0, math.cos(c), -math.sin(c)], [0, math.sin(c), math.cos(c)]], F)
    R = np.zeros((3, 3), F)
    for i in range(3):
        for j in range(3):
            R[i, j] = (Ry[i, 0] * Rx[0, j] + Ry[i, 1] * Rx[1, j]) + Ry[i, 2] * Rx[2, j]
    t = np.array([0.1, -0.05, 0.2], F)
    Ow = np.array([-((R[0, k] * t[0] + R[1, k] * t[1]) + R[2, k] * t[2]) for k in range(3)], F)
    for b in range(3):
        items[b] = (R.ravel(), t, Ow, 458.654, 457.296, 367.215, 248.375, 47.90639, (0, 0, 752, 480), 0, (0, 0, 0))
    # item 3: identity, tcw = -0.0 (x + -0.0 = x for every x, and -0.0 stays -0.0), a principal point near the corner and the undistorted
    # bounds of a 752 x 480 image, so that u - cx and u lie in one binade at all four edges and every edge value can be hit exactly
    items[3] = (np.eye(3, dtype=F).ravel(), F(-0.0) * np.ones(3, F), np.zeros(3, F), 458.654, 457.296, 7.215, 8.375, 47.90639,
                (-135.79564, -92.87501, 895.50732, 565.55316), 0, (0, 0, 0))
    it3 = items[3]

    # ---- the random part: around the camera of item 2, mostly inside the viewing cone
    for i in range(NRANDOM):
        z = F(-0.5 - rng.randint(300) * 0.01) if i % 11 == 5 else F(0.6 + rng.randint(800) * 0.01)
        P = np.array([(rng.randint(2000) - 1000) * 0.001 * z * 0.95, (rng.randint(2000) - 1000) * 0.001 * z * 0.62, z], F)
        n = P - Ow
        nn = F(np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]))
        normal = n / nn + (rng.rand(3) * 0.4 - 0.2).astype(F)
        if i % 7 == 3:
            normal = -normal                                     # the viewing-angle gate
        maxd = F(nn * F(0.7 + rng.randint(200) * 0.01))          # the distance gate cuts both ways
        mind = F(maxd / F(1.6)) if i % 9 == 4 else F(maxd / F(4.3))
        points[i] = (P, F(0.8) * mind, normal, F(1.2) * maxd, maxd, (0, 0, 0))
        obs[i] = rng.randint(1, 9)
    obs[7] = obs[29] = -1                                        # isBad()
    obs[13] = 0                                                  # a point nobody observes is not bad

    # ---- the planted part, in the camera coordinates of item 3
    planted, rows = {}, []

    def plant(name, P, exit_, min_inv=0.0, max_inv=None, normal=None, max_dist=None, observations=3):
        i = NRANDOM + len(rows)
        P = np.array(P, F)
        d = float(np.sqrt(np.sum(P.astype(np.float64) ** 2)))
        if normal is None:                                       # along the viewing ray: viewCos is 1 or a float beside it
            normal = P.astype(np.float64) / d if d > 0 else (0, 0, 1)
        max_dist = F(max(d, 1e-30)) if max_dist is None else F(max_dist)
        points[i] = (P, F(min_inv), np.array(normal, F), F(1.2) * max_dist if max_inv is None else F(max_inv), max_dist, (0, 0, 0))
        obs[i] = observations
        rows.append(i)
        planted[name] = (3, len(rows) - 1, exit_)
        return i

    def trace(P, **kw):
        """The model's trace of a scratch point under item 3."""
        tab, o = np.zeros(1, fm.TABLE_DTYPE), np.ones(1, np.int32)
        P = np.array(P, F)
        tab[0] = (P, 0, kw.get("normal", (0, 0, 1)), kw.get("max_inv", np.inf), kw.get("max_dist", 1), (0, 0, 0))
        return fm.project_slot(it3, tab, o, 0, lsf, NLEVELS, COS_LIMIT, fm.SUM_LTR, fm.LOG_DOUBLE)

    # depth: -0.0f is not below zero and goes on (to a u of +inf); the largest negative float returns
    plant("pcz_minus_zero", (-0.1, -0.1, -0.0), fm.U)
    z = trace((-0.1, -0.1, -0.0))[4]["Pc"][2]
    assert z == 0 and np.signbit(z) and np.isposinf(trace((-0.1, -0.1, -0.0))[4]["u"])
    plant("pcz_largest_negative", (0.0, 0.0, -1e-45), fm.DEPTH)
    # image bounds: exactly on each edge (passes), the next float outside (fails).  z = 1: u = fl(fx * x) + cx, non-decreasing in x
    minx, miny, maxx, maxy = it3["bounds"]
    fu = lambda x: trace((x, 0, 1))[4]["u"]                      # noqa: E731
    fv = lambda y: trace((0, y, 1))[4]["v"]                      # noqa: E731
    for name, f, axis, edge, beyond, why in (("u_min", fu, 0, minx, down(minx), fm.U), ("u_max", fu, 0, maxx, up(maxx), fm.U),
                                             ("v_min", fv, 1, miny, down(miny), fm.V), ("v_max", fv, 1, maxy, up(maxy), fm.V)):
        for tag, target, exit_ in (("_on", edge, fm.ACCEPTED), ("_beyond", beyond, why)):
            x = solve(f, target, F(-4), F(4))
            plant(name + tag, (x, 0, 1) if axis == 0 else (0, x, 1), exit_)
    # distance: P = (0, 0, 2), dist = 2 exactly
    plant("dist_at_min", (0, 0, 2), fm.ACCEPTED, min_inv=2.0)
    plant("dist_below_min", (0, 0, 2), fm.DISTANCE, min_inv=up(2.0))
    plant("dist_at_max", (0, 0, 2), fm.ACCEPTED, max_inv=2.0, max_dist=2.0)
    plant("dist_above_max", (0, 0, 2), fm.DISTANCE, max_inv=down(2.0), max_dist=2.0)
    # viewing angle: viewCos = (2 * nz) / 2 = nz exactly
    plant("cos_at_limit", (0, 0, 2), fm.ACCEPTED, normal=(0, 0, COS_LIMIT))
    plant("cos_below_limit", (0, 0, 2), fm.ANGLE, normal=(0, 0, down(COS_LIMIT)))
    # levels: ratio = max_dist / 2 exactly.  Every threshold of both log kinds and the next float above it
    for kind, tag in ((fm.LOG_DOUBLE, "d"), (fm.LOG_FLOAT, "f")):
        for n in range(NLEVELS - 1):
            T = threshold(lsf, n, kind)
            plant("ratio_T%d%s" % (n, tag), (0, 0, 2), fm.ACCEPTED, max_dist=T * F(2))
            plant("ratio_T%d%s_up" % (n, tag), (0, 0, 2), fm.ACCEPTED, max_dist=up(T) * F(2))
    plant("ratio_far_above", (0, 0, 2), fm.ACCEPTED, max_dist=200.0)
    plant("ratio_below_one", (0, 0, 2), fm.ACCEPTED, max_dist=1.8)
    # dist = 0: P = Ow.  u, v and viewCos are NaN (0 / 0) and pass every comparison, the ratio is infinite: level 0
    plant("dist_zero", (0, 0, 0), fm.ACCEPTED, max_dist=1.0)
    # operands for which fma(-mbf, invz, u) differs from the product and the subtraction, and for which (fx * x) * invz differs from
    # (fx * x) / z: found by search
    need = {"xr_not_fused": None, "u_divides": None}
    while any(v is None for v in need.values()):
        P = np.array([rng.rand() * 2 - 1, rng.rand() - 0.5, 1 + rng.rand() * 3], F)
        tr = trace(P)
        if tr[3] != fm.ACCEPTED:
            continue
        u, invz = tr[4]["u"], tr[4]["invz"]
        fused = F(float(Fraction(float(u)) - Fraction(float(it3["mbf"])) * Fraction(float(invz))))
        if need["xr_not_fused"] is None and fused != tr[0][2]:
            need["xr_not_fused"] = P
        if need["u_divides"] is None and (it3["fx"] * P[0]) * invz + it3["cx"] != u:
            need["u_divides"] = P
    for name, P in need.items():
        plant(name, P, fm.ACCEPTED)
    # coordinates whose squares are subnormal
    plant("subnormal_squares", (1e-20, 1.5e-20, 2e-20), fm.ACCEPTED, normal=(0.4, 0.5, 0.7), max_dist=9e-20)
    tr = trace((1e-20, 1.5e-20, 2e-20))
    assert all(0 < s < np.finfo(F).tiny for s in tr[4]["Pc_sq"]), tr[4]["Pc_sq"]
    # isBad() and never-observed points among the planted ones
    plant("bad_point", (0, 0, 2), fm.SKIPPED, observations=-1)
    plant("bad_point_2", (0.1, 0, 2), fm.SKIPPED, observations=-7)
    plant("unobserved_point", (0, 0.1, 2), fm.ACCEPTED, observations=0)
    assert NRANDOM + len(rows) <= NPOINTS, len(rows)
    for i in range(NRANDOM + len(rows), NPOINTS):                # the rest of the table: plain points in front of the identity camera
        P = np.array([rng.rand() - 0.5, rng.rand() * 0.6 - 0.3, 1.5 + 4 * rng.rand()], F)
        d = F(np.sqrt((P[0] * P[0] + P[1] * P[1]) + P[2] * P[2]))
        maxd = F(d * F(1 + 3 * rng.rand()))
        points[i] = (P, F(0.8) * F(maxd / F(4.3)), P / d, F(1.2) * maxd, maxd, (0, 0, 0))
        obs[i] = rng.randint(1, 9)

    # ---- the lists
    idx[0] = np.arange(MCAP) + 10 ** 6                           # nmp = 0: none of it is read
    nmp[0] = 0
    idx[1] = rng.randint(0, NPOINTS, MCAP)
    idx[1, 57] = NPOINTS                                         # one past the table
    nmp[1] = 100
    idx[2] = rng.permutation(np.r_[np.arange(NRANDOM), np.arange(NPOINTS - 20, NPOINTS)])[:MCAP]
    idx[2, [4, 77]] = (-1, -5)                                   # slots the caller wants skipped
    idx[2, MCAP - 1] = 10 ** 6                                   # beyond nmp: not read
    nmp[2] = MCAP - 1
    row = list(rows)
    row += [-1, -2, -(2 ** 31)]                                  # negative indices
    row += [rows[5], rows[5], rows[20], NPOINTS - 1, NPOINTS - 1]   # repeated indices
    row += list(range(NPOINTS - 1, NPOINTS - 1 - (MCAP - len(row)), -1))
    assert len(row) == MCAP
    idx[3] = row
    nmp[3] = MCAP
    # far_th of item 2: between two accepted depths
    _, depth, _, exits = fm.project(points, obs, items, idx, nmp, lsf, NLEVELS, COS_LIMIT)
    d = np.sort(depth[2][exits[2] == fm.ACCEPTED])
    assert len(d) >= 8 and d[len(d) // 2 - 1] < d[len(d) // 2]
    items[2]["far_th"] = F((d[len(d) // 2 - 1] + d[len(d) // 2]) / F(2))
    for a_ in (points, obs, items, idx, nmp):
        a_.setflags(write=False)                                 # shared among the tests: left unchanged
    return dict(points=points, obs=obs, items=items, idx=idx, nmp=nmp, lsf=lsf, planted=planted)


@functools.lru_cache(maxsize=None)
def expected(sum_order: int, log_kind: int):
    """The model's (mp, depth, ntomatch, exits) for the batch, computed once per option pair."""
    b = batch()
    return fm.project(b["points"], b["obs"], b["items"], b["idx"], b["nmp"], b["lsf"], NLEVELS, COS_LIMIT, sum_order, log_kind)
