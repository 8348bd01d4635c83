#!/usr/bin/env python3
"""Batched two-camera rig matcher times (liborbx_rigmatch.so) -> profiles/rigmatch_times_r24.txt.

  python tools/rigmatch_times.py [--items 256] [--features 1500] [--points 2000] [--repeats 15] [--out PATH]

The shape: `--items` TUM-VI-shaped pairs (512 x 512, `--features` keypoints a side, about `--points` local points an item), a SYNTHETIC
side: keypoints drawn in clusters, random descriptors, every third left keypoint paired with a right one; the points are the item's own
keypoints (left ones, then right ones) with drift and noise, as tests/test_gpu_rigmatch.py draws them.  No image is extracted.
  rig_local / rig_last   orbx_rigmatch_local_device / orbx_rigmatch_last_device, HIP events on one stream, `--repeats` runs after three
                         warm-up runs: median [min, max]; kp_obs is restored (a device copy) outside the bracket before every run
  left_local / left_last LocalMatchBatch / LastMatchBatch on the LEFT side alone with the left halves of the same rows: what the second
                         camera and the coupled chain cost
  split                  both rig calls once more on a timing build of the same source without phase B (-DORBX_RIGMATCH_NO_CHAIN): what is
                         left is the parallel part; the chain's share = 1 - that / the whole
  adapter_local / adapter_last  the per-frame loop through the drop-in adapter's rig path (csrc/ref_adapter/ORBmatcher.cc over liborbx.so)
                         on the same inputs: tools/rig_adapter_loop.cpp builds a rig Frame an item from these arrays and calls, as Tracking
                         does on a new frame, SearchByProjection(Cur, Last) (the frame becomes resident here) and then SearchByProjection(Cur,
                         map points); wall clock around the matcher calls alone, summed over the items, median [min, max] of `--passes`
                         passes.  Entry 2's rows are the ones that program's caller part computed, and both paths' results are compared.
  scaling                the rig calls at 2x and 4x the items (the same frames and rows again): whether the chain's share costs throughput"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from times_util import stats, write_result  # noqa: E402
OUT = os.path.join(ROOT, "profiles", "rigmatch_times_r24.txt")
SIZE, SHIFT = 512, 24


def no_chain_library_path():
    """The timing build: the library's one source with phase B compiled out, beside the objects of the in-tree build."""
    from orb_slam3_modified_amd import build
    src = os.path.join(build.CSRC, build.RIGMATCH_SOURCE)
    out = os.path.join(os.path.dirname(build.OUT), "build", "liborbx_rigmatch_nochain.so")
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        flags = [f for f in build.FLAGS if f != "-ldl"] + ["-fvisibility=hidden", "-DORBX_RIGMATCH_NO_CHAIN"]
        subprocess.check_call([os.environ.get("HIPCC", "hipcc")] + flags + [src, "-o", out, "-ldl"])
    return out


def adapter_loop_path():
    """tools/rig_adapter_loop.cpp over the drop-in adapter and liborbx.so, beside the objects of the in-tree build."""
    from orb_slam3_modified_amd import build
    from tests import world_util as wu
    build.build()
    src = os.path.join(ROOT, "tools", "rig_adapter_loop.cpp")
    out = os.path.join(os.path.dirname(build.OUT), "build", "rig_adapter_loop.bin")
    if wu._stale(out, wu._deps() + [src, os.path.join(wu.PKG, "liborbx.so")]):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++"] + wu.CXXFLAGS + wu.INCLUDES + ["-I", wu.SUP, src, wu.ADAPTER_SRC, "-o", out, "-DORBX_NO_CV_CALIBRATION", "-L", wu.PKG,
                               "-lorbx", "-Wl,-rpath," + wu.PKG, "-Wl,--allow-shlib-undefined"])
    return out


def write_records(path, recs):
    import struct
    with open(path, "wb") as f:
        for name, a in recs.items():
            a = np.ascontiguousarray(a)
            kind = 0 if a.dtype == np.int32 else 1 if a.dtype == np.float32 else 2
            f.write(struct.pack("<i", len(name)) + name.encode() + struct.pack("<ii", kind, a.size if kind < 2 else a.nbytes) + a.tobytes())


def run_adapter(exe, tmp, hs, mp, pts, pool, obs0, sf, B, n, npts, passes):
    """-> the program's records: the LastFrame rows its caller part computed, both calls' ids and return values, a pass's ms."""
    from tests.rigmatch_world import read_dump
    spec = np.zeros((B, npts), np.dtype([("u", "<f4"), ("v", "<f4"), ("angle", "<f4"), ("octave", "<i4"), ("obs", "<i4"), ("point", "<i4"), ("valid", "<i4")]))
    for k in spec.dtype.names:
        spec[k] = pts[k]
    inp, out = os.path.join(tmp, "rig_adapter_in.bin"), os.path.join(tmp, "rig_adapter_out.bin")
    write_records(inp, {"shape": np.array([B, n, npts, SIZE], np.int32), "sf": sf, "call": np.array([3.0, 0.8, 15.0, SHIFT], np.float32),
                        "kps_l": hs["kps_l"].view(np.uint8), "kps_r": hs["kps_r"].view(np.uint8), "desc_l": hs["desc_l"], "desc_r": hs["desc_r"],
                        "pdesc": pool, "l2r": hs["l2r"], "r2l": hs["r2l"], "kp_obs": obs0, "mp": mp.view(np.uint8), "last_spec": spec.view(np.uint8)})
    subprocess.run([exe, inp, out, str(passes)], check=True, timeout=900)
    return read_dump(out)


def ids_of(kp_match, kp_obs0, slots):
    """A batched result as the adapter prints it: the point's index where the call bound one, NULL where the rotation filter removed
    one, otherwise the pre-bound point (900000 + slot) or NULL."""
    held = np.where(kp_obs0 >= 0, 900000 + np.arange(slots)[None], -1)
    return np.where(kp_match >= 0, kp_match, np.where(kp_match == -2, -1, held))


def make_side(rng, B, n):
    from orb_slam3_modified_amd._lib import KP_DTYPE
    side = {}
    centres = rng.uniform(20, SIZE - 20, (B, n // 3 + 1, 2))
    xy = centres[:, np.arange(n) % centres.shape[1]] + rng.normal(0, 4.0, (B, n, 2))
    octave = rng.choice([0, 0, 0, 1, 1, 2, 2, 3, 4, 5, 6, 7], (B, n))
    desc = rng.integers(0, 256, (B, n, 32)).astype(np.uint8)
    for cam, dx in (("l", 0.0), ("r", -float(SHIFT))):
        k = np.zeros((B, n), KP_DTYPE)
        k["x"], k["y"], k["octave"], k["angle"], k["size"] = np.clip(xy[..., 0] + dx, 1, SIZE - 2), np.clip(xy[..., 1], 1, SIZE - 2), octave, \
            rng.uniform(0, 360, (B, n)), 31.0
        d = desc.copy()
        flips = rng.integers(0, 32, (B, n, 2))
        np.put_along_axis(d, flips, np.take_along_axis(d, flips, 2) ^ rng.integers(0, 256, (B, n, 2)).astype(np.uint8), 2)
        side["kps_" + cam], side["desc_" + cam], side["counts_" + cam] = k, d, np.tile(np.array([[n, 0]], np.int32), (B, 1))
    l2r = np.where(np.arange(n) % 3 == 0, np.arange(n), -1).astype(np.int32)
    side["l2r"], side["r2l"] = np.tile(l2r, (B, 1)), np.tile(l2r, (B, 1))
    side["bounds"] = np.tile(np.array([[0, 0, SIZE, SIZE]], np.float32), (B, 1))
    return side


def make_rows(rng, side, B, n, npts):
    from orb_slam3_modified_amd.rigmatch import LAST_ITEM_DTYPE, LAST_POINT_DTYPE, LOCAL_POINT_DTYPE
    mp, pts = np.zeros((B, npts), LOCAL_POINT_DTYPE), np.zeros((B, npts), LAST_POINT_DTYPE)
    pick = np.stack([rng.permutation(2 * n)[:npts] for _ in range(B)])           # < n: a left keypoint, else right keypoint pick - n
    right = pick >= n
    idx = np.where(right, pick - n, pick)
    k = np.where(right, np.take_along_axis(side["kps_r"], idx, 1), np.take_along_axis(side["kps_l"], idx, 1))
    x = k["x"] + np.where(right, SHIFT, 0) + rng.normal(0, 1.0, (B, npts))
    y = k["y"] + rng.normal(0, 1.0, (B, npts))
    mp["proj_x"], mp["proj_y"], mp["proj_xr"], mp["proj_yr"] = x, y, x - SHIFT, y + rng.normal(0, 0.5, (B, npts))
    mp["view_cos"], mp["view_cos_r"] = rng.choice([0.9, 0.9995], (B, npts)), rng.choice([0.9, 0.9995], (B, npts))
    mp["level"] = np.clip(k["octave"] + rng.integers(-1, 2, (B, npts)), 0, 7)
    mp["level_r"] = np.where(rng.random((B, npts)) < 0.08, -1, mp["level"])
    mp["obs"], mp["in_view"], mp["in_view_r"] = rng.choice([0, 2, 2], (B, npts)), rng.random((B, npts)) < 0.8, rng.random((B, npts)) < 0.75
    mp["point"] = np.arange(B)[:, None] * 2 * n + pick                               # the pool: every frame's left rows, then its right rows
    for a, b in (("u", "proj_x"), ("v", "proj_y"), ("u_r", "proj_xr"), ("v_r", "proj_yr"), ("obs", "obs"), ("point", "point")):
        pts[a] = mp[b]
    pts["angle"], pts["octave"], pts["valid"] = k["angle"] + rng.normal(0, 3.0, (B, npts)), k["octave"], rng.random((B, npts)) < 0.85
    items = np.zeros(B, LAST_ITEM_DTYPE)
    items["frame"], items["direction"], items["th"] = np.arange(B), 0, 15.0
    pool = np.concatenate([side["desc_l"], side["desc_r"]], 1).reshape(-1, 32)
    return mp, pts, items, pool


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=256)
    ap.add_argument("--features", type=int, default=1500)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--passes", type=int, default=3, help="passes of the adapter loop")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--build-only", action="store_true", help="make the timing build and stop (no device is touched)")
    args = ap.parse_args()
    nochain, adapter = no_chain_library_path(), adapter_loop_path()
    if args.build_only:
        return
    import torch
    from orb_slam3_modified_amd import build
    from orb_slam3_modified_amd.lastmatch import ITEM_DTYPE as L_ITEM, POINT_DTYPE as L_POINT, LastMatchBatch, LastMatchSide
    from orb_slam3_modified_amd.localmatch import POINT_DTYPE as M_POINT, LocalMatchBatch, LocalMatchSide
    from orb_slam3_modified_amd.rigmatch import LDS_MAX, RigMatchBatch, RigSide, lds_bytes
    import tempfile
    B, n, npts = args.items, args.features, args.points
    rng = np.random.default_rng(24)
    hs = make_side(rng, B, n)
    mp, pts, items, pool = make_rows(rng, hs, B, n, npts)
    sf = np.cumprod(np.concatenate([[1.0], np.full(7, 1.2)])).astype(np.float32)
    h_obs0 = rng.choice([-1, -1, -1, 0, 2], (B, 2 * n)).astype(np.int32)
    # (a) first, in a process of its own: the adapter loop; entry 2 then runs on the rows its caller part computed
    with tempfile.TemporaryDirectory() as tmp:
        ad = run_adapter(adapter, tmp, hs, mp, pts, pool, h_obs0, sf, B, n, npts, args.passes)
    rf, ri = ad["rows_f"].reshape(B, npts, 5), ad["rows_i"].reshape(B, npts, 3)
    for k, name in enumerate(("u", "v", "u_r", "v_r", "angle")):
        pts[name] = rf[..., k]
    for k, name in enumerate(("octave", "obs", "valid")):
        pts[name] = ri[..., k]
    dev = torch.device("cuda", 0)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (-1,)) if a.dtype.names else np.ascontiguousarray(a)).to(dev)   # noqa: E731
    t = {k: to(v) for k, v in hs.items()}
    side = RigSide(t["kps_l"], t["desc_l"], t["counts_l"], t["kps_r"], t["desc_r"], t["counts_r"], t["l2r"], t["r2l"], t["bounds"], B, n, n)
    frames, nrows = to(np.arange(B, dtype=np.int32)), to(np.full(B, npts, np.int32))
    d_mp, d_pts, d_items, d_pool = to(mp), to(pts), to(items), to(pool)
    obs0 = to(h_obs0)
    obs = obs0.clone()
    stream = torch.cuda.Stream(device=dev)
    res = {"stamp": build.stamp(), "shape": {"items": B, "image": [SIZE, SIZE], "features_per_side": n, "points_per_item": npts, "side": "synthetic"},
           "lds_bytes_needed": lds_bytes(n, n, npts) + 4 * 2 * n}
    limit = max(0, min(LDS_MAX, int(os.environ.get("ORBX_RIGMATCH_LDS", LDS_MAX)))) & ~15   # what orbx_rigmatch_create reads; plan_paths' test
    res["lds_limit"], res["path"] = limit, "lds" if res["lds_bytes_needed"] <= limit else "global"

    def bracket(fn):
        ts = []
        for _ in range(args.repeats + 3):
            with torch.cuda.stream(stream):
                obs.copy_(obs0)
            ts.append(_one(stream, fn))
        return stats(ts[3:])

    def _one(st, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1)

    outs = {}
    for name, path in (("", None), ("split_without_phase_b_", nochain)):
        rb = RigMatchBatch(0, path) if path else RigMatchBatch(0)
        o1 = rb.search_local_points_device(side, frames, d_mp, nrows, d_pool, sf, obs, 3.0, 0.8, stream=stream.cuda_stream)
        res[name + "rig_local_ms"] = bracket(lambda: rb.search_local_points_device(side, frames, d_mp, nrows, d_pool, sf, obs, 3.0, 0.8, stream=stream.cuda_stream, out=o1))
        o2 = rb.search_last_frame_device(side, d_items, d_pts, nrows, d_pool, sf, obs, True, stream=stream.cuda_stream)
        res[name + "rig_last_ms"] = bracket(lambda: rb.search_last_frame_device(side, d_items, d_pts, nrows, d_pool, sf, obs, True, stream=stream.cuda_stream, out=o2))
        stream.synchronize()
        if not path:
            outs["local"], outs["last"] = o1.nmatches.cpu().numpy().copy(), o2.nmatches.cpu().numpy().copy()
            for e, o, after in (("local", o1, False), ("last", o2, True)):   # the bracket's last run left o1; o2 is the loop's last call
                if not after:
                    with torch.cuda.stream(stream):
                        obs.copy_(obs0)
                    rb.search_local_points_device(side, frames, d_mp, nrows, d_pool, sf, obs, 3.0, 0.8, stream=stream.cuda_stream, out=o1)
                    stream.synchronize()
                same_ids = np.array_equal(ids_of(o.kp_match.cpu().numpy(), h_obs0, 2 * n), ad["ids_" + e].reshape(B, 2 * n))
                res["adapter_equal_" + e] = bool(same_ids and np.array_equal(o.nmatches.cpu().numpy(), ad["ret_" + e]))
            # at 2x and 4x the items
            for mult in (2, 4):
                fx, nx = to(np.tile(np.arange(B, dtype=np.int32), mult)), to(np.full(B * mult, npts, np.int32))
                mx, px, ix = to(np.tile(mp, (mult, 1))), to(np.tile(pts, (mult, 1))), to(np.tile(items, mult))
                ox0 = to(np.tile(h_obs0, (mult, 1)))
                ox = ox0.clone()
                for e, call in (("local", lambda out=None: rb.search_local_points_device(side, fx, mx, nx, d_pool, sf, ox, 3.0, 0.8, stream=stream.cuda_stream, out=out)),
                                ("last", lambda out=None: rb.search_last_frame_device(side, ix, px, nx, d_pool, sf, ox, True, stream=stream.cuda_stream, out=out))):
                    keep, ts = call(), []
                    for _ in range(args.repeats + 3):
                        with torch.cuda.stream(stream):
                            ox.copy_(ox0)
                        ts.append(_one(stream, lambda: call(keep)))
                    res["scaling_%dx_rig_%s_ms" % (mult, e)] = stats(ts[3:])
                del fx, nx, mx, px, ix, ox0, ox
        rb.close()
    for e in ("local", "last"):
        whole, rest = res["rig_%s_ms" % e]["median"], res["split_without_phase_b_rig_%s_ms" % e]["median"]
        res["chain_share_of_rig_" + e] = round(1.0 - rest / whole, 3)
    res["matches_per_item_median"] = {k: int(np.median(v)) for k, v in outs.items()}
    assert (outs["local"] >= 0).all() and (outs["last"] >= 0).all()
    # (b) the left side alone through the one-camera matchers: the left halves of the same rows
    m1 = np.zeros((B, npts), M_POINT)
    for k in ("proj_x", "proj_y", "view_cos", "level", "obs", "in_view"):
        m1[k] = mp[k]
    m1["point"] = mp["point"]
    l1 = np.zeros((B, npts), L_POINT)
    l1["u"], l1["v"], l1["invz"], l1["angle"], l1["octave"], l1["obs"], l1["point"], l1["valid"] = pts["u"], pts["v"], 0.2, pts["angle"], pts["octave"], \
        pts["obs"], pts["point"], pts["valid"]
    li = np.zeros(B, L_ITEM)
    li["frame"], li["direction"], li["mbf"], li["th"] = np.arange(B), 0, 40.0, 15.0
    obs_l0 = obs0[:, :n].contiguous()
    obs_l = obs_l0.clone()

    def bracket_left(fn):
        ts = []
        for _ in range(args.repeats + 3):
            with torch.cuda.stream(stream):
                obs_l.copy_(obs_l0)
            ts.append(_one(stream, fn))
        return stats(ts[3:])

    lb = LocalMatchBatch(0)
    ls = LocalMatchSide(t["kps_l"], t["desc_l"], t["counts_l"], t["bounds"], B, n)
    d_m1 = to(m1)
    o = lb.search_device(ls, frames, d_m1, nrows, d_pool, sf, obs_l, 3.0, 0.8, stream=stream.cuda_stream)
    res["left_local_ms"] = bracket_left(lambda: lb.search_device(ls, frames, d_m1, nrows, d_pool, sf, obs_l, 3.0, 0.8, stream=stream.cuda_stream, out=o))
    lb.close()
    kb = LastMatchBatch(0)
    ks = LastMatchSide(t["kps_l"], t["desc_l"], t["counts_l"], t["bounds"], B, n)
    d_l1, d_li = to(l1), to(li)
    o = kb.search_device(ks, d_li, d_l1, nrows, d_pool, sf, obs_l, True, stream=stream.cuda_stream)
    res["left_last_ms"] = bracket_left(lambda: kb.search_device(ks, d_li, d_l1, nrows, d_pool, sf, obs_l, True, stream=stream.cuda_stream, out=o))
    stream.synchronize()
    kb.close()
    for e in ("local", "last"):
        res["rig_over_left_" + e] = round(res["rig_%s_ms" % e]["median"] / res["left_%s_ms" % e]["median"], 2)
    for e in ("local", "last"):
        res["adapter_%s_ms" % e] = stats(ad["ms_" + e])
        res["adapter_over_rig_" + e] = round(res["adapter_%s_ms" % e]["median"] / res["rig_%s_ms" % e]["median"], 2)
    write_result(args.out, "tools/rigmatch_times.py: batched two-camera rig matchers, HIP-event medians [min, max] of --repeats runs (ms)", res)


if __name__ == "__main__":
    main()
