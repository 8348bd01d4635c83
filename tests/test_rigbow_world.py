"""tests/rigbow_model.py against the reference (CPU only): the recorded bow_kf_frame_rig / bow_kf_kf_rig lines of the golden world, the
reference binary on a second world where it is built, and the drop-in adapter's rig SearchByBoW (oracle backend) on the same frames --
all on the scenarios' objects as tests/support/rig_bow_dump.cpp rebuilds them in include/orbx_rigbow.h's layout."""
import gzip
import os

import numpy as np
import pytest

from tests import rigbow_model as rm
from tests import rigbow_world as rw
from tests import world_util as wu


def _model_on(rec):
    out = {}
    for name in rw.SCENARIOS:
        b = rw.batch(rec, name)
        n, b2a, a2b = rw.model(b)
        out[name] = (n, rw.ids_line(b, b2a, a2b), b, a2b)
    return out


def _same(got, want):
    for name in rw.SCENARIOS:
        assert got[name][0] == want[name][0], (name, got[name][0], want[name][0])
        assert len(got[name][1]) == len(want[name][1]) and np.array_equal(got[name][1], want[name][1]), name


@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("rigbow_world")
    gold = rw.recorded(gzip.open(os.path.join(wu.ROOT, "tests", "golden", "matcher_world_ref.txt.gz")).read().decode())
    return gold, rw.dump(rw.golden_world(tmp), tmp)


def test_the_model_equals_the_recorded_lines(golden):
    gold, rec = golden
    assert set(gold) == set(rw.SCENARIOS) and all(gold[n][0] > 50 for n in gold)
    got = _model_on(rec)
    _same(got, gold)
    # the scenarios reach what is the rig's own: capacities above the counts, right features on both sides, and in frame mode keyframe
    # features that hold two slots and right-camera keyframe features that are queries
    n, _, b, a2b = got["bow_kf_frame_rig"]
    assert b["a"]["capacity"] > b["a"]["n"] > b["a"]["nleft"][0] > 0 and b["b"]["capacity"] > b["b"]["n"] > b["b"]["nleft"][0] > 0
    assert ((a2b >= 0).sum(1) == 2).sum() > 0 and (a2b[b["a"]["nleft"][0]:] >= 0).any() and (a2b[:, 1] >= 0).sum() > 0
    n, ids, b, a2b = got["bow_kf_kf_rig"]
    assert len(ids) == b["a"]["n"] and (a2b[:, 1] == -1).all() and not (a2b[b["a"]["nleft"][0]:] >= 0).any()
    assert b["a"]["valid"][0, b["a"]["nleft"][0]:b["a"]["n"]].any() and b["b"]["valid"][0, b["b"]["nleft"][0]:b["b"]["n"]].any()   # :800, :820 gate something


def test_the_model_equals_the_adapter_on_the_same_frames(golden):
    """The drop-in adapter's rig SearchByBoW (oracle backend), run by the dump program on the very objects it wrote."""
    gold, rec = golden
    got = _model_on(rec)
    for name in rw.SCENARIOS:
        ret, ids = got[name][2]["adapter"]
        assert got[name][0] == ret and np.array_equal(got[name][1], ids), name
        assert ret == gold[name][0] and np.array_equal(ids, gold[name][1]), name   # the dump's objects are the scenarios'


def test_the_model_equals_the_reference_on_another_world(tmp_path):
    from tests.test_matcher_world import OTHER_WORLDS
    if not os.path.exists(wu.REF_EXE):
        pytest.skip("oracle/_ref/ref_matcher_world not built (needs the reference)")
    kw = dict(OTHER_WORLDS[0], rows=512, cols=512, nfeatures=400)
    world = str(tmp_path / "world.bin")
    wu.write_world(world, **kw)
    ref = rw.recorded(wu.run_world(wu.REF_EXE, world, str(tmp_path / "ref.txt"), only="bow_kf_"))
    assert set(ref) == set(rw.SCENARIOS) and ref["bow_kf_frame_rig"][0] > 20
    _same(_model_on(rw.dump(world, tmp_path)), ref)
