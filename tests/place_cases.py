"""Constructed inputs of the batched place recognition (include/orbx_place.h), stated once: tests/test_place_model.py holds the model
to the oracle on every one of them and shows that each planted world depends on its rule, tests/test_gpu_place.py runs them on the
device.  A world is a dict: db (rows in add() order, None = erased), kf_map, kf_cov [D, 10], score_in float32 [D], q (queries), q_map,
excl (per query, N-best), n (nNumCandidates), ccap.  With positive values the L1 score of a pair is the sum over the common words of
min(query value, row value); the values here are dyadic, so every score below is exact.  Deterministic; nothing here needs a GPU."""
import numpy as np

from tests import place_model as pm

STRIDE = 48                  # the device layout's stride in the GPU tests (rows of 0, 1 and STRIDE entries occur)
LDS_LOW = 40                 # ORBX_PLACE_LDS in the size-edge runs: queries of 39, 40 and 41 entries straddle it
SIZE_EDGES = [(1, 1), (63, 5), (64, 1), (65, 5), (257, 5)]   # (D, Q)


def vec(ids, vals):
    ids = np.asarray(ids, np.int64)
    assert len(ids) == len(vals) and (len(ids) < 2 or (np.diff(ids) > 0).all())
    return ids.astype(np.uint32), np.asarray(vals, np.float64)


def flat(ids, v=1.0 / 16):
    return vec(ids, [v] * len(ids))


def cov_rows(D, rows=None):
    c = np.full((D, pm.COV), -1, np.int32)
    for d, r in (rows or {}).items():
        c[d, :len(r)] = r
    return c


def world(name, db, q, kf_map=None, cov=None, score_in=None, q_map=None, excl=None, n=3, ccap=8, rule=None, kinds=(pm.RELOC, pm.NBEST)):
    D, Q = len(db), len(q)
    return dict(name=name, db=db, q=q, kf_map=np.zeros(D, np.int32) if kf_map is None else np.asarray(kf_map, np.int32),
                kf_cov=cov_rows(D, cov), score_in=np.zeros(D, np.float32) if score_in is None else np.asarray(score_in, np.float32),
                q_map=np.zeros(Q, np.int32) if q_map is None else np.asarray(q_map, np.int32), excl=excl or [[] for _ in range(Q)], n=n, ccap=ccap,
                rule=rule, kinds=kinds)


R = lambda a, b: list(range(a, b))   # noqa: E731


def planted():
    """name -> world; world["rule"]: the model rules (place_model.DROPS) whose loss changes the world's result."""
    w = []
    # row 0 scored (10 of 10 words), row 1 in the query (5 words <= min 8) with IN score 5: it takes row 0's holder and lifts acc above
    # what row 2 (9 words, alone) can reach
    w.append(world("unscored_neighbour_in", [flat(R(0, 10)), flat(R(0, 5)), flat(R(1, 10))], [flat(R(0, 10))], cov={0: [1]},
                   score_in=[0, 5, 0], rule=("unscored_neighbour",)))
    # the same, but the 5 is what query 0 of the call leaves in row 1; the IN array holds 0
    w.append(world("unscored_neighbour_earlier_query", [flat(R(0, 10)), flat(R(0, 5) + R(20, 30), 8.0), flat(R(1, 10))],
                   [flat(R(20, 30), 0.5), flat(R(0, 10))], cov={0: [1]}, rule=("earlier_query", "unscored_neighbour")))
    # rows 0-3 the same vector: equal si, equal acc.  Row 4 holds the query's lowest word: first in the list although last in the database
    w.append(world("equal_acc_and_first_word", [flat(R(1, 9))] * 4 + [flat([0] + R(2, 9))], [flat(R(0, 9))], n=2,
                   rule=("stable_sort", "tie_by_row", "first_word")))
    # maxCommonWords 5, 10, 15: (int)(max * 0.8f) = 4, 8, 12 and the rows with exactly that many words are not scored
    db = [flat(R(0, 5)), flat(R(0, 4)), flat(R(100, 110)), flat(R(100, 108)), flat(R(100, 109)), flat(R(200, 215)), flat(R(200, 212)),
          flat(R(200, 213))]
    w.append(world("truncation_5_10_15", db, [flat(R(0, 5)), flat(R(100, 110)), flat(R(200, 215))], rule=("truncation", "strict_threshold")))
    # rows 0 and 1 both reach row 2 (in the query, IN score 3) as their holder; row 3, first in the list, is held by row 4 of another map
    # with IN score 4, ahead of the holders of the query's own map
    db = [flat(R(1, 11)), flat(R(1, 11)), flat(R(1, 4)), flat(R(0, 10)), flat(R(1, 3))]
    w.append(world("holder_twice_and_other_map_first", db, [flat(R(0, 11))], kf_map=[0, 0, 0, 0, 1], cov={0: [2], 1: [2], 3: [4]},
                   score_in=[0, 0, 3, 0, 4], rule=("dedup", "map")))
    # six candidates of the query's map and five of another, ccap 3
    w.append(world("ccap_below_count", [flat(R(0, 8))] * 6 + [flat(R(0, 8), 1.0 / 32)] * 5, [flat(R(0, 8))], kf_map=[0] * 6 + [1] * 5, n=5, ccap=3,
                   rule=("full_count",)))
    # an empty query, a query whose rows are all excluded (N-best), an ordinary one; row 1 is erased and would have been the best row
    db = [flat(R(0, 6)), None, flat(R(0, 5)), flat(R(30, 40))]
    w.append(world("empty_erased_excluded", db, [vec([], []), flat(R(0, 6)), flat(R(0, 6) + R(30, 40))], excl=[[], [0, 2], [3]],
                   rule=("exclusion",)))
    # cov rows with -1 between entries and a row that lists itself: acc0 = 9/16 + 9/16 passes acc1 = 10/16 only through the self entry
    db = [flat(R(0, 9)), flat(R(0, 10))]
    wd = world("cov_padding_and_self", db, [flat(R(0, 10))], rule=("self_neighbour",))
    wd["kf_cov"][0, :4] = (-1, 0, -1, -1)
    wd["kf_cov"][1, :3] = (-1, -1, -1)
    w.append(wd)
    return {x["name"]: x for x in w}


def size_edge(D, Q, seed=20271):
    """Random rows over a small vocabulary (many common words, many ties): rows of 0, 1 and STRIDE entries, queries of LDS_LOW - 1, LDS_LOW and
    LDS_LOW + 1 entries among them, two maps, random covisibility (self entries and padding included), random IN scores and exclusions."""
    rng = np.random.default_rng(seed + 1000 * D + Q)
    words = np.arange(0, 3 * 120, 3)

    def draw(n):
        ids = np.sort(rng.choice(words, n, replace=False))
        return vec(ids, rng.integers(1, 9, n) / 64.0)

    lens = [STRIDE, 1, 0] + [int(x) for x in rng.integers(2, STRIDE, max(D - 3, 0))]
    db = [draw(n) for n in lens[:D]]
    if D > 4:
        db[4] = None
        db[D - 1] = (db[0][0].copy(), db[0][1].copy())          # a duplicate of the full row
    qlens = [LDS_LOW, LDS_LOW - 1, LDS_LOW + 1, 1, STRIDE]
    q = [draw(n) for n in qlens[:Q]]
    cov = np.full((D, pm.COV), -1, np.int32)
    for d in range(D):
        k = int(rng.integers(0, pm.COV + 1))
        cov[d, :k] = rng.integers(0, D, k)
        if k > 2:
            cov[d, 1] = -1
    excl = [sorted(set(int(x) for x in rng.integers(0, D, int(rng.integers(0, 4))))) for _ in range(Q)]
    wd = world("edge_%d_%d" % (D, Q), db, q, kf_map=rng.integers(0, 2, D), score_in=(rng.integers(0, 64, D) / 32.0).astype(np.float32),
               q_map=rng.integers(0, 2, Q), excl=excl, n=3, ccap=4)
    wd["kf_cov"] = cov
    return wd


def run_model(kind, w, drop=None):
    return pm.run(kind, w["db"], w["kf_map"], w["kf_cov"], w["score_in"], w["q"], w["q_map"], w["excl"], w["n"], w["ccap"], drop)


def same(a, b):
    """Two results of run(): every array equal, scores by bits."""
    for k in ("cand", "ncand", "merge", "nmerge", "stats"):
        if (a[k] is None) != (b[k] is None) or (a[k] is not None and not np.array_equal(a[k], b[k])):
            return False
    return np.array_equal(np.asarray(a["score"], np.float32).view(np.uint32), np.asarray(b["score"], np.float32).view(np.uint32))
