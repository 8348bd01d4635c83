"""The GPU KeyFrameDatabase (k_kfdb_common / k_kfdb_score and their host code, orb_slam3_modified_amd/csrc/orbx_kfdb.hip) at the sizes where it
changes path, on the constructed scripts of tests/kfdb_edge_cases.py (tests/test_kfdb_edge_cases.py checks on the CPU that each of them is
what it claims and that a wrong kernel could not pass it): queries of 1 .. 65 words, at 5461 / 5462 words where k_kfdb_score's staging passes
64 KB of LDS, at 8191 .. 8193 where the query moves from LDS to HBM; rows of 0 .. 20 000 words with their hits placed lane by lane; 1 .. 5
rows and a row table grown past its first 1024 rows; the erase at which the host mirror is compacted; ties in the list order; thresholds
from 12 down to nothing; scores of widely spread values, -0.0 among them.  The product and the oracle run every script in lockstep and every
answer is compared byte for byte."""
import ctypes as C

import numpy as np
import pytest

from orb_slam3_modified_amd import KeyFrameDatabase, ORBextractor
from orb_slam3_modified_amd._lib import ptr
from tests import kfdb_edge_cases as kc
from tests.test_gpu_kfdb import _same

pytestmark = pytest.mark.gpu

ORBX_E_CAPACITY = -4          # include/orbx.h


@pytest.fixture(scope="module")
def ex():
    return ORBextractor(500, 1.2, 6, 20, 7, device_id=0)   # the context the databases live on; nothing is extracted


def _lockstep(db, odb, steps):
    """Every step on both; the script is handed the oracle's answer.  -> the number of answers compared."""
    n = [0]

    def run(step):
        got, want = kc.apply(db, step), kc.apply(odb, step)
        where = (n[0], step[0])
        if step[0] == "query":
            _same(got, want)
            assert not set(step[2]) & set(got["kf"].tolist()), where
        elif step[0] == "sharing":                                 # the oracle's unexcluded query
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), where
        elif step[0] == "score":                                   # po.score_l1, pair by pair
            assert got.dtype == np.float64 and got.tobytes() == want.tobytes(), (where, got, want)
        else:
            assert len(db) == len(odb), where
        n[0] += step[0] in ("query", "sharing", "score")
        return want

    kc.drive(steps, run)
    return n[0]


@pytest.mark.parametrize("name", sorted(kc.CASES))
def test_kfdb_edge_case(ex, name):
    db = KeyFrameDatabase(ex)
    assert _lockstep(db, kc.OracleDb(), kc.CASES[name]()) >= 7
    db.close()


def test_kfdb_capacity_one_below_the_list(ex):
    """orbx_kfdb_sharing / orbx_kfdb_query with room for one keyframe less than share a word: ORBX_E_CAPACITY, and the database answers the
    same call with enough room as if nothing had happened."""
    p = kc.thresholds_plan()
    db, odb = KeyFrameDatabase(ex), kc.OracleDb()
    for i in p.add_order:
        db.add(p.kfs[i][0], p.kfs[i][2]); odb.add(p.kfs[i][0], p.kfs[i][2])
    want = odb.query(p.query, [], 0)
    full = len(want["kf"])
    assert full == 24 < len(db)
    L = db._L
    ids, vals = np.ascontiguousarray(p.query[0], np.uint32), np.ascontiguousarray(p.query[1], np.float64)
    for cap in (full - 1, full):
        kf = np.full(full, -77, np.int64); words = np.full(full, -77, np.int32); score = np.full(full, -77.0)
        n, mx, mn = C.c_int(-1), C.c_int(-1), C.c_int(-1)
        rc = L.orbx_kfdb_sharing(db._db, ptr(ids), len(ids), ptr(kf), ptr(words), cap, C.byref(n))
        assert n.value == full                                     # set even when the capacity is too small (include/orbx.h)
        if cap < full:
            assert rc == ORBX_E_CAPACITY
        else:
            assert rc == 0 and np.array_equal(kf, want["kf"]) and np.array_equal(words, want["words"])
        kf[:] = -77; words[:] = -77
        rc = L.orbx_kfdb_query(db._db, ptr(ids), ptr(vals), len(ids), None, 0, 0, ptr(kf), ptr(words), ptr(score), cap, C.byref(n), C.byref(mx),
                               C.byref(mn))
        if cap < full:
            assert rc == ORBX_E_CAPACITY and kf[cap] == -77 and score[cap] == -77.0      # nothing written past the capacity
        else:
            assert rc == 0 and n.value == full
            _same(dict(kf=kf, words=words, score=score, max_common=mx.value, min_common=mn.value), want)
    _same(db.query(p.query, [], 0), want)
    db.close()
