"""One constructed batch for the batched SearchByBoW (include/orbx_match.h): 15 pairs over 17 small frames with hand-written FeatureVectors,
capacity 256.  A node is a site: the "already matched" dependence never leaves it, so every edge of the specification is planted in a node
of its own, both sides of an edge where it has two.  numpy only: the CPU test (tests/test_match_batch_model.py) holds the batch to its
claims on tests/match_batch_model.py and, in frame mode, to the oracle; the GPU test (tests/test_gpu_match_batch.py) runs it on every path.

A call has one mode, one nn_ratio and one form of `valid` for all its pairs: every pair goes through every combination (whole rows), and a
claim names the nn_ratio (RUNS) it was built for and gives its outcome as a function of (mode, valid given).

PLANTED[name] = the A feature, KP[name] = the B feature the site is about, CLAIMS[name] = (pair, run, want(mode, valid given) -> a KP name
or None): what a2b holds for the A feature."""
import numpy as np

from orb_slam3_modified_amd._lib import KP_DTYPE
from tests.initmatch_cases import bin_edge, desc, ratio_triple

FRAME, KEYFRAMES = 0, 1
CAP = 256
(MA, MB, E1, E2, E3, E5, NOFV, WA, WB1, WB2, WB3, RA1, RA2, RB, NEGCOUNT, NEGFV, BADFEAT) = range(17)
K = 17
(P_PLANT, P_DISJOINT, P_BADFRAME, P_FIRST, P_LAST, P_NOFV_B, P_BADCOUNT, P_W1, P_W2, P_W3, P_BADFV, P_ROT1, P_ROT2, P_BADFEAT, P_NOFV_A) = range(15)
PAIRS = np.array([(MA, MB), (E1, E2), (E1, K), (E1, E3), (E1, E5), (E1, NOFV), (NEGCOUNT, MB), (WA, WB1), (WA, WB2), (WA, WB3), (MA, NEGFV),
                  (RA1, RB), (RA2, RB), (BADFEAT, E3), (NOFV, E1)], np.int32)
MALFORMED = {P_BADFRAME: "frame", P_BADCOUNT: "negative count", P_BADFV: "negative fv_n", P_BADFEAT: "fv_feat entry at its frame's count"}
BEST, SECOND, RATIO = ratio_triple()                             # float32(SECOND) * float32(RATIO) rounds to exactly BEST, from above
RUNS = {"main": RATIO, "low": 0.1, "high": 1.5}
N_WAVE = {"nb_1": 1, "nb_63": 63, "nb_64": 64, "nb_65": 65, "nb_129": 129, "lane_pair": 72, "lane_pair_twin": 72}   # B candidates of the nodes


class _Frame:
    def __init__(self):
        self.kps, self.desc, self.valid, self.n, self.fv = np.zeros(CAP, KP_DTYPE), np.zeros((CAP, 32), np.uint8), np.ones(CAP, np.uint8), 0, {}

    def add(self, d, angle=0.0, valid=1):
        i = self.n
        assert i < CAP
        self.kps[i]["angle"], self.kps[i]["size"], self.valid[i] = angle, 31.0, valid
        self.desc[i] = desc(d) if np.isscalar(d) else d
        self.n += 1
        return i

    def arrays(self):
        node, ptr, feat = np.zeros(CAP, np.uint32), np.zeros(CAP + 1, np.int32), np.zeros(CAP, np.uint32)
        k = 0
        for j, nid in enumerate(sorted(self.fv)):
            node[j] = nid
            feat[k:k + len(self.fv[nid])] = self.fv[nid]
            k += len(self.fv[nid])
            ptr[j + 1] = k
        ptr[len(self.fv) + 1:] = k
        return node, ptr, feat, len(self.fv)


def build():
    """-> dict(kps [K, CAP], desc, counts [K, 2], fv_node [K, CAP], fv_ptr [K, CAP + 1], fv_feat [K, CAP], fv_n [K], valid [K, CAP],
    fv: the K FeatureVectors as dicts node -> list, pairs [15, 2]) and fills PLANTED / KP / CLAIMS."""
    fr = [_Frame() for _ in range(K)]
    PLANTED.clear(); KP.clear(); CLAIMS.clear()
    always, never = (lambda mode, valid: True), (lambda mode, valid: False)   # noqa: E731

    def claim(name, pair, run, a, b, want=always):
        PLANTED[name], KP[name] = a, b
        CLAIMS[name] = (pair, run, lambda mode, valid: (lambda w: name if w is True else (None if not w else w))(want(mode, valid)))

    A, B = fr[MA], fr[MB]
    nid = iter(range(10, 1000, 3))

    def node(a_feats, b_feats):
        n = next(nid)
        A.fv[n], B.fv[n] = list(a_feats), list(b_feats)

    # ---- (a) bestDist1 50: taken towards a frame, not between keyframes; 49 in both modes, 51 in neither
    for name, d, want in (("th_50", 50, lambda mode, valid: mode == FRAME), ("th_49", 49, always), ("th_51", 51, never)):
        a, b = A.add(0), B.add(d)
        node([a], [b])
        claim(name, P_PLANT, "main", a, b, want)
    # ---- (b) a lone candidate meets 256 (not INT_MAX): at nn_ratio 0.1 distance 25 passes 25.6 and 26 does not (run "low")
    for name, d in (("single_25", 25), ("single_26", 26)):
        a, b = A.add(0), B.add(d)
        node([a], [b])
        claim(name, P_PLANT, "low", a, b, always if d == 25 else never)
    a, b = A.add(0), B.add(256)                                  # the complement: distance 256 is "no candidate", even alone, at any ratio
    node([a], [b])
    claim("complement", P_PLANT, "high", a, b, never)
    for name, d in (("ratio_at", BEST), ("ratio_under", BEST - 1)):   # the ratio at float32 equality, and one bit closer
        a, b = A.add(0), B.add(d)
        node([a], [b, B.add(SECOND)])
        claim(name, P_PLANT, "main", a, b, always if d < BEST else never)
    # ---- (c) a tie goes to the first in fv_feat order (written descending here); with nn_ratio < 1 the tie is the second best too
    a, b1, b2 = A.add(0), B.add(5), B.add(5)
    node([a], [b2, b1])
    claim("tie", P_PLANT, "high", a, b2)
    claim("tie_ratio", P_PLANT, "main", a, b2, never)
    KP["tie:lower_index"] = b1
    # the A features of a node in fv_feat order (descending here): the first takes X, the second skips it and takes the runner-up ...
    a2, a1, x, y = A.add(1), A.add(0), B.add(0), B.add(8)
    node([a1, a2], [x, y])
    claim("first_takes", P_PLANT, "main", a1, x)
    claim("runner_up", P_PLANT, "main", a2, y)
    # ... or fails the ratio among the survivors (30 against 32) where the first passed it (0 against 30)
    a1, a2, x, y, z = A.add(0), A.add(0), B.add(0), B.add(30), B.add(32)
    node([a1, a2], [x, y, z])
    claim("first_takes_2", P_PLANT, "main", a1, x)
    claim("second_fails", P_PLANT, "main", a2, y, never)
    # ---- (d) an A feature with valid 0 is skipped (when the flags are given)
    a, b = A.add(0, valid=0), B.add(0)
    node([a], [b])
    claim("invalid_a", P_PLANT, "main", a, b, lambda mode, valid: not valid)
    # a B feature with valid 0 that would have been the best: between keyframes the next one is taken; a frame's flags are ignored
    a, x, y, z = A.add(0), B.add(5, valid=0), B.add(30), B.add(120)
    node([a], [x, y, z])
    claim("invalid_b_best", P_PLANT, "main", a, x, lambda mode, valid: "invalid_b_best:next" if (mode == KEYFRAMES and valid) else True)
    KP["invalid_b_best:next"] = y
    # ---- (e) a node on A only and one on B only, between common ones
    A.fv[next(nid)] = [A.add(0)]
    B.fv[next(nid)] = [B.add(0)]
    a, b = A.add(0), B.add(3)
    node([a], [b])
    claim("after_one_sided_nodes", P_PLANT, "main", a, b)
    # the node lists: E1 {1, 5, 9} against E2 {2, 6, 10} (disjoint), E3 {1, 6, 10} (the first only), E5 {2, 6, 9} (the last only), no list
    for f, nodes in ((E1, (1, 5, 9)), (E2, (2, 6, 10)), (E3, (1, 6, 10)), (E5, (2, 6, 9)), (BADFEAT, (1, 5, 9))):
        for n in nodes:
            fr[f].fv[n] = [fr[f].add(0)]
    for i, (name, pair) in enumerate((("first_node_only", P_FIRST), ("last_node_only", P_LAST))):
        claim(name, pair, "main", 2 * i, 2 * i)
        claim(name + ":others", pair, "main", 1, 1, never)
    claim("disjoint", P_DISJOINT, "main", 0, 0, never)
    for f in (NOFV, NEGCOUNT, NEGFV):
        for _ in range(3):
            fr[f].add(0)
    fr[NEGCOUNT].fv[1] = [0]; fr[NEGFV].fv[1] = [0]
    claim("no_fv_on_b", P_NOFV_B, "main", 0, 0, never)
    claim("no_fv_on_a", P_NOFV_A, "main", 0, 0, never)

    # ---- (f) the wave-node boundary: nodes of 1, 63, 64, 65 and 129 B candidates; list positions run against the feature indices
    W = fr[WA]

    def wave_node(f, n, nb, special, a_feats):
        idx = [0] * nb                                           # position j holds feature idx[j]: descending indices
        for j in reversed(range(nb)):
            idx[j] = fr[f].add(special.get(j, 100 + j % 50))
        fr[f].fv[n] = [idx[j] for j in range(nb)]
        for j, d in special.items():
            assert np.unpackbits(fr[f].desc[idx[j]]).sum() == d
        W.fv[n] = list(a_feats)
        return idx
    idx = wave_node(WB1, 100, 1, {0: 10}, [W.add(0)])
    claim("nb_1", P_W1, "main", W.fv[100][0], idx[0])
    # the minimum stands twice; the lower list position wins (run "high": the tie is accepted).  In the 65 and 129 nodes the two stand on
    # different trips and the later position on the lower lane
    for name, f, pair, n, nb, lo, hi in (("nb_63", WB1, P_W1, 163, 63, 2, 40), ("nb_64", WB1, P_W1, 164, 64, 3, 63), ("nb_65", WB1, P_W1, 165, 65, 10, 64),
                                         ("nb_129", WB2, P_W2, 229, 129, 70, 128)):
        idx = wave_node(f, n, nb, {lo: 20, hi: 20}, [W.add(0)])
        claim(name, pair, "high", W.fv[n][0], idx[lo])
        claim(name + "_ratio", pair, "main", W.fv[n][0], idx[lo], never)
        KP[name + ":later"], KP[name + ":positions"] = idx[hi], (lo, hi)
    # best (position 7) and second (position 71) on one lane, nothing else within the ratio: rejected; the second made farther: accepted
    idx = wave_node(WB2, 172, 72, {7: 20, 71: 22}, [W.add(0)])
    claim("lane_pair", P_W2, "main", W.fv[172][0], idx[7], never)
    idx = wave_node(WB3, 173, 72, {7: 20, 71: 100}, [W.add(0)])
    claim("lane_pair_twin", P_W3, "main", W.fv[173][0], idx[7])
    # 70 A features over 4 B features: the first four distinct ones take them all, the long rest finds every candidate taken
    idx = wave_node(WB3, 300, 4, {0: 0, 1: 9, 2: 18, 3: 27}, [W.add(9 * (i % 4)) for i in range(70)])
    for i in range(4):
        claim("chain_%d" % i, P_W3, "main", W.fv[300][i], idx[i])
    claim("chain_late", P_W3, "main", W.fv[300][69], idx[1], never)

    # ---- (g) rotation: 48 one-feature nodes on RB, angle 0 but where a site needs a negative difference
    e11, e12 = bin_edge(11)
    for i in range(48):
        fr[RB].fv[1000 + i] = [fr[RB].add(0, angle={40: 5.0, 42: 20.0}.get(i, 0.0))]
    # P_ROT1: bin sizes 30, 3, 2, 1.  float32 0.1f * 30 is 3.0: the 3 stays, the 2 goes; the lone bin 11 is none of the three
    R = fr[RA1]
    for i in range(30):
        R.fv[1000 + i] = [R.add(0, angle=0.0)]
    claim("rot_bin0", P_ROT1, "main", 29, 29)
    for name, i, a, keep in (("rot_negative", 40, 0.0, True), ("rot_at_edge", 41, e12, True), ("rot_negative_2", 42, 10.0, True), ("rot_two_a", 43, 180.0, False),
                             ("rot_two_b", 44, 180.0, False), ("rot_under_edge", 45, e11, False)):
        R.fv[1000 + i] = [R.add(0, angle=a)]
        claim(name, P_ROT1, "main", R.fv[1000 + i][0], i, (lambda k: lambda mode, valid: k)(keep))
    # P_ROT2: four bins of two; bin 0 holds a rotation of 900 (bin 30 -> 0): the strict > keeps bins 0, 3, 6 and drops bin 9.  Without the
    # fold bin 0 holds one and goes, bin 9 stays
    R = fr[RA2]
    for name, i, a, keep in (("rot_fold", 0, 900.0, True), ("rot_0", 1, 0.0, True), ("rot_3a", 2, 90.0, True), ("rot_3b", 7, 90.0, True), ("rot_6a", 3, 180.0, True),
                             ("rot_6b", 4, 180.0, True), ("rot_9a", 5, 270.0, False), ("rot_9b", 6, 270.0, False)):
        R.fv[1000 + i] = [R.add(0, angle=a)]
        claim(name, P_ROT2, "main", R.fv[1000 + i][0], i, (lambda k: lambda mode, valid: k)(keep))

    arrays = [f.arrays() for f in fr]
    c = dict(kps=np.stack([f.kps for f in fr]), desc=np.stack([f.desc for f in fr]), counts=np.array([[f.n, 0] for f in fr], np.int32),
             fv_node=np.stack([a[0] for a in arrays]), fv_ptr=np.stack([a[1] for a in arrays]), fv_feat=np.stack([a[2] for a in arrays]),
             fv_n=np.array([a[3] for a in arrays], np.int32), valid=np.stack([f.valid for f in fr]), fv=[dict(f.fv) for f in fr], pairs=PAIRS.copy())
    c["counts"][NEGCOUNT, 0] = -1
    c["fv_n"][NEGFV] = -1
    c["fv_feat"][BADFEAT, 1] = fr[BADFEAT].n                      # the first value that is not below the frame's count
    assert c["fv_n"][NOFV] == 0 and c["counts"][NOFV, 0] > 0 and len(PAIRS) <= 16
    return c


def frame(c, f):
    """Frame f's (descriptors, angles, valid flags, FeatureVector)."""
    n = int(c["counts"][f, 0])
    return c["desc"][f, :n], c["kps"][f, :n]["angle"], c["valid"][f, :n], c["fv"][f]


PLANTED, KP, CLAIMS = {}, {}, {}
