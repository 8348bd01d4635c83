"""CPU guard of tests/test_gpu_many_levels.py's inputs: every configuration fills EVERY pyramid level in the oracle, so that a GPU result that
equals the oracle's cannot be one with empty upper levels; and the stereo / SearchByProjection inputs really reach octaves 8 and 9."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import many_levels_util as mu


@pytest.mark.parametrize("cfg", mu.MANY_LEVELS, ids=lambda c: "%dx%d-nf%d-sf%g-L%d" % c)
def test_every_level_holds_keypoints_in_the_oracle(cfg):
    rows, cols, nf, sf, nlev = cfg
    assert 9 <= nlev <= 16
    t = mu.oracle(cfg).tables()
    assert len(t["quota"]) == nlev and (t["quota"] >= 1).all()
    top = mu.level_size(rows, cols, t["inv_scale"], nlev - 1)
    assert min(top) >= 67, top
    kps, desc, mono = mu.want(cfg)
    cnt = np.bincount(kps["octave"], minlength=nlev)
    assert len(cnt) == nlev and (cnt >= 1).all(), cnt.tolist()
    assert mu.oracle(cfg).level(nlev - 1).shape == top
    if (rows, cols) == (346, 346):
        assert top == (67, 67)
    if (rows, cols) == (1040, 1300):
        assert 0 < mono < len(kps)


def test_the_table_holds_the_issue_s_shapes():
    assert len(mu.MANY_LEVELS) == 7 and (300, 400, 800, 1.2, 9) in mu.MANY_LEVELS
    assert sorted({c[4] for c in mu.MANY_LEVELS}) == [9, 10, 12, 16]


def test_stereo_pairs_match_on_the_two_top_octaves():
    """The oracle alone (its own levels as the pyramids): some left keypoint of octave >= 8 finds its right partner, so the sub-pixel
    refinement reads a level-8 or level-9 plane on both sides."""
    L, R, _ = mu.stereo_pairs()
    cfg = mu.STEREO
    nlev = cfg["params"][2]
    oL, oR = po.OracleExtractor(*cfg["params"]), po.OracleExtractor(*cfg["params"])
    t = oL.tables()
    hits = 0
    for f in range(len(L)):
        kL, dL, _ = oL.extract(L[f], (0, 0))
        kR, dR, _ = oR.extract(R[f], (0, 0))
        ur, dp, kept = po.stereo_matches(kL, dL, kR, dR, [oL.level(l) for l in range(nlev)], [oR.level(l) for l in range(nlev)],
                                         t["scale"], t["inv_scale"], cfg["mb"], cfg["mbf"])
        assert kept > 0
        hits += int(((kL["octave"] >= 8) & (ur >= 0)).sum())
    assert hits > 0


def test_search_by_projection_inputs_accept_matches_on_the_two_top_octaves():
    fr = mu.projection_frames()
    ora = po.OracleExtractor(*mu.PROJ_PARAMS)
    sf = ora.tables()["scale"]
    assert len(sf) == 10
    F = []
    for img in fr:
        k, d, _ = ora.extract(img, mu.LAP)
        F.append(mu.Frame(k, d, (0.0, 0.0, float(img.shape[1]), float(img.shape[0]))))
    for stereo in (False, True):
        mp, kp_obs, ur = mu.projection_case(F[0], F[1], sf, stereo, 30 + stereo)
        n, match, _ = po.search_by_projection(F[1].mvKeysUn, F[1].mDescriptors, F[1].bounds, sf, kp_obs, mp, 3.0, 0.8, ur)
        assert n > 200 and ((match >= 0) & (F[1].mvKeysUn["octave"] >= 8)).sum() > 0 and mp["level"].max() == 9
