"""The two-sided staging of the four pair matchers' host forms (csrc/side/orbx_pair_host.h: stage_sides, device_sides) on the GPU: each
library's constructed batch through its host form equals its device form on uploaded copies, word for word, with one object on both sides,
with two objects whose structs compare equal, and with two batches of different capacities whose optional arrays are present on one side
and null on the other -- on the LDS path and under the library's ORBX_*_LDS=0, where the shared tail grows the scratch."""
import copy

import numpy as np
import pytest

from orb_slam3_modified_amd.initmatch import InitMatchBatch, InitSide
from orb_slam3_modified_amd.match import FRAME, KEYFRAMES, MatchBatch, MatchSide
from orb_slam3_modified_amd.rigbow import RigBowBatch, RigBowSide
from orb_slam3_modified_amd.trimatch import TriMatchBatch, TriMatchSide
from tests import initmatch_cases as ic
from tests import match_batch_cases as mc
from tests import rigbow_cases as rc
from tests import trimatch_cases as tc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PER_FRAME = ("counts", "fv_n", "nleft")


def _dev():
    return torch.device("cuda", 0)


def _to(a):
    """A host array on the device: keypoint records as bytes, uint32 as its int32 bits."""
    a = np.ascontiguousarray(a)
    if a.dtype.names:
        a = a.view(np.uint8).reshape(a.shape + (-1,))
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(_dev())


def _recap(arrays, cap):
    """The same frames in arrays of a larger capacity: zero rows behind each frame's own, fv_ptr's new entries its last one."""
    out = {}
    for name, a in arrays.items():
        if name in PER_FRAME:
            out[name] = a.copy()
        else:
            wide = np.zeros((a.shape[0], cap + (name == "fv_ptr")) + a.shape[2:], a.dtype)
            wide[:, :a.shape[1]] = a
            if name == "fv_ptr":
                wide[:, a.shape[1]:] = a[:, -1:]
            out[name] = wide
    return out


def _sides(cls, arrays, cap, other_cap, optional):
    """(a, b) on the host: the batch at `cap` and the same frames at `other_cap`; a has the first optional array and not the others, b the
    others and not the first."""
    base = arrays if arrays["desc"].shape[1] == cap else _recap(arrays, cap)
    other = arrays if arrays["desc"].shape[1] == other_cap else _recap(arrays, other_cap)
    F = len(base["counts"])
    on_a = {n: base[n] for n in base if n not in optional[1:]}
    on_b = {n: other[n] for n in other if n not in optional[:1]}
    return cls(nframes=F, capacity=cap, **base), cls(nframes=F, capacity=cap, **on_a), cls(nframes=F, capacity=other_cap, **on_b)


def _uploaded(side):
    return side.__class__(**{k: (_to(v) if isinstance(v, np.ndarray) else v) for k, v in vars(side).items()})


def _match():
    c = mc.build()
    arrays = {n: c[n] for n in MatchSide._FIELDS}
    pairs = mc.PAIRS[:6]
    host = lambda h, a, b: h.bow_pairs(a, b, pairs, KEYFRAMES, mc.RATIO, True)                                     # noqa: E731
    device = lambda h, a, b, s: h.bow_pairs_device(a, b, _to(pairs), KEYFRAMES, mc.RATIO, True, stream=s)           # noqa: E731
    return MatchBatch, "ORBX_MATCH_LDS", _sides(MatchSide, arrays, mc.CAP, mc.CAP + 64, ("valid",)), host, device, ("nmatches", "b2a", "a2b")


def _rigbow():
    c = rc.build()
    arrays = {n: c[n] for n in RigBowSide._FIELDS}
    pairs = rc.PAIRS[:6]
    host = lambda h, a, b: h.bow_pairs(a, b, pairs, FRAME, rc.RATIO, True)                                         # noqa: E731
    device = lambda h, a, b, s: h.bow_pairs_device(a, b, _to(pairs), FRAME, rc.RATIO, True, stream=s)               # noqa: E731
    return RigBowBatch, "ORBX_RIGBOW_LDS", _sides(RigBowSide, arrays, rc.CAP, rc.CAP + 64, ("valid", "nleft")), host, device, ("nmatches", "b2a", "a2b")


def _trimatch():
    from tests.test_gpu_trimatch import CAP, _constructed, _pack
    from tests.test_trimatch_model import FREE, LINE_X0
    kps, desc, counts, fvs, has, ur, _ = _constructed()
    node, ptr, feat, n = _pack(fvs, CAP)
    arrays = dict(kps=kps, desc=desc, counts=counts, fv_node=node, fv_ptr=ptr, fv_feat=feat, fv_n=n, has_point=has, uright=ur)
    pairs = np.array([(0, 1), (1, 0), (0, 0), (1, 1), (0, 2), (2, 1)], np.int32)
    geom = np.stack([LINE_X0, tc.geometry_of("sideways"), tc.geometry_of("forward"), tc.geometry_of("forward"), FREE, FREE]).astype(np.float32)
    scale, sig = tc.level_tables()
    host = lambda h, a, b: h.pairs(a, b, pairs, geom, scale, sig, False, False, True)                              # noqa: E731
    device = lambda h, a, b, s: h.pairs_device(a, b, _to(pairs), _to(geom), scale, sig, False, False, True, stream=s)   # noqa: E731
    return TriMatchBatch, "ORBX_TRIMATCH_LDS", _sides(TriMatchSide, arrays, 256, CAP, ("has_point", "uright")), host, device, ("nmatches", "matches12")


def _initmatch():
    c = ic.build()
    arrays = {n: c[n] for n in InitSide._FIELDS}
    pairs, prev = ic.PAIRS[:6], c["prev"][:6]
    window, ratio, bounds = ic.RUNS["main"]
    host = lambda h, a, b: h.pairs(a, b, pairs, bounds, window, ratio, True, prev_xy=prev)                         # noqa: E731
    device = lambda h, a, b, s: h.pairs_device(a, b, _to(pairs), bounds, window, ratio, True, prev_xy=_to(prev), stream=s)   # noqa: E731
    return InitMatchBatch, "ORBX_INITMATCH_LDS", _sides(InitSide, arrays, ic.CAP, ic.CAP + 64, ()), host, device, ("nmatches", "matches12", "matches21", "prev_xy")


LIBRARIES = {"match": _match, "rigbow": _rigbow, "trimatch": _trimatch, "initmatch": _initmatch}


@pytest.fixture(scope="module", params=list(LIBRARIES))
def library(request):
    return request.param, LIBRARIES[request.param]()


@pytest.mark.parametrize("path", ["lds", "global"])
def test_the_host_form_stages_what_the_device_form_reads(library, monkeypatch, path):
    name, (batch, env, (whole, a, b), host, device, rows) = library
    if path == "global":
        monkeypatch.setenv(env, "0")
    h = batch(0)
    monkeypatch.delenv(env, raising=False)
    s = torch.cuda.Stream(device=_dev())
    twin = copy.copy(whole)                                          # another object, the same arrays: its struct compares equal
    assert twin is not whole and bytes(twin._host()._struct()) == bytes(whole._host()._struct())
    assert bytes(a._host()._struct()) != bytes(b._host()._struct()) and a.capacity != b.capacity
    for staging, (x, y) in (("b is a", (whole, whole)), ("equal structs", (whole, twin)), ("two batches", (a, b))):
        dx = _uploaded(x)
        dy = dx if y is x or y is twin else _uploaded(y)
        torch.cuda.synchronize()
        want = device(h, dx, dy, s.cuda_stream)
        s.synchronize()
        got = host(h, x, y)
        for row in rows:
            g, w = np.asarray(getattr(got, row)), getattr(want, row).cpu().numpy()
            assert g.shape == w.shape and g.tobytes() == w.tobytes(), (name, path, staging, row)
        assert (np.asarray(got.nmatches) > 0).any(), (name, path, staging)
    h.close()
