#!/usr/bin/env python3
"""Batched relocalization and Sim3 SearchByProjection times (liborbx_projmatch.so) -> profiles/projmatch_times_r18.txt.

256 synthetic frames at the EuRoC shape (752 x 480; 1000 features, 1.2, 8 levels, 20 / 7) resident in HBM, their descriptors the pool.
  reloc   every frame against 8 candidate keyframes (its 8 predecessors: their keypoints as the keyframe's map points, drift growing with
          the distance, noise, angles turned by a few degrees, some by anything): 2048 items of kind 0, the rotation check on, run at
          (th, ORBdist) = (10, 100) and again at (3, 64) with the keypoints the first run bound taken, as Tracking::Relocalization does
  sim3    every frame as a keyframe against ~2000 points (the keypoints of its two predecessors): 256 items of kind 1 at (8, 1.5)
For each:
  (a) orbx_projmatch_search_device, HIP events on one stream, `--repeats` runs after three warm-up runs: median [min, max]
  (b) the per-call loop of ORBmatcher.SearchByProjectionReloc / SearchByProjectionSim3 (matcher.py: one WindowSearchGrid call and the host
      chain in Python per item) over the first `--percall` items, wall clock, median of three; its results are checked against the batched
      rows in the same run; `lists_only`: the WindowSearchGrid calls alone (upload, device pass, download: what the adapter's C++ chain
      would add almost nothing to).  The whole loop's time is the per-item time times the item count: an extrapolation, named as one
  split: (a) once more on a timing build of the same source without phase B (-DORBX_PROJMATCH_NO_CHAIN): the difference is the chain's share
  (d) the batch extraction that feeds (a), HIP events
"""
from __future__ import annotations

import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from times_util import Extracted, stats, write_result  # noqa: E402
OUT = os.path.join(ROOT, "profiles", "projmatch_times_r18.txt")
LASTMATCH_R17_MS = 0.352      # profiles/lastmatch_times_r17.txt: 256 items of ~906 valid points


def timing_library_path(name, define):
    """A timing build: the library's one source with a phase compiled out, beside the objects of the in-tree build."""
    from orb_slam3_modified_amd import build
    src = os.path.join(build.CSRC, build.PROJMATCH_SOURCE)
    out = os.path.join(os.path.dirname(build.OUT), "build", "liborbx_projmatch_%s.so" % name)
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        flags = [f for f in build.FLAGS if f != "-ldl"] + ["-fvisibility=hidden", "-D" + define]
        subprocess.check_call([os.environ.get("HIPCC", "hipcc")] + flags + [src, "-o", out, "-L", os.path.dirname(build.OUT),
                                                                            "-l:" + os.path.basename(build.OUT), "-Wl,-rpath," + os.path.dirname(build.OUT), "-ldl"])
    return out


def projected(rng, hk, hc, sources, B, cap, mcap):
    """A row of POINT_DTYPE: the keypoints of the frames `sources` = [(g, drift)] as map points projected into the item's frame."""
    from orb_slam3_modified_amd.projmatch import POINT_DTYPE
    row = np.zeros(mcap, POINT_DTYPE)
    k = 0
    for g, drift in sources:
        n = min(int(hc[g, 0]), mcap - k)
        kg, r = hk[g, :n], row[k:k + n]
        r["valid"] = rng.random(n) < 0.9
        r["u"] = kg["x"] + drift + rng.normal(0, 1.5, n)
        r["v"] = kg["y"] + 0.2 * drift + rng.normal(0, 1.5, n)
        r["angle"] = np.where(rng.random(n) < 0.9, (kg["angle"] + rng.normal(3, 8, n)) % 360, rng.uniform(0, 360, n))
        r["level"] = kg["octave"]
        r["point"] = g * cap + np.arange(n)
        k += n
    return row, k


class _F:
    pass


def per_call(om, x, bounds, sf, items, pts, npts, taken, got, count):
    """(b): the per-call methods over the first `count` items, checked against the batched rows -> (whole loop, lists only) in ms."""
    hp = x.hd.reshape(-1, 32)
    jobs = []
    for b in range(count):
        f, k = int(items[b]["frame"]), int(npts[b])
        n = int(x.hc[f, 0])
        r = pts[b, :k]
        fr = _F()
        fr.mvKeysUn, fr.mDescriptors, fr.bounds, fr.mvScaleFactors = np.ascontiguousarray(x.hk[f, :n]), np.ascontiguousarray(x.hd[f, :n]), bounds[f], sf
        fr.kp_taken = None if taken is None else taken[b, :n]
        pp = dict(desc=np.ascontiguousarray(hp[r["point"]]), **{key: np.ascontiguousarray(r[key]) for key in ("valid", "u", "v", "angle", "level")})
        jobs.append((fr, pp, n))

    def one(b):
        it = items[b]
        fr, pp, n = jobs[b]
        if it["kind"] == 0:
            return om.SearchByProjectionReloc(fr, pp, float(it["th"]), int(it["max_dist"]))
        return om.SearchByProjectionSim3(fr, pp, int(it["th"]), float(it["max_dist"]) / om.TH_LOW)

    whole, lists = [], []
    for rep in range(4):
        t0 = time.perf_counter()
        res = [one(b) for b in range(count)]
        whole.append((time.perf_counter() - t0) * 1e3)
        if rep == 0:
            for b, (nm, match) in enumerate(res):
                n = jobs[b][2]
                assert nm == got[0][b] and np.array_equal(match, got[1][b, :n]), ("batched != per-call", b)
        t0 = time.perf_counter()
        for b in range(count):
            fr, pp, n = jobs[b]
            live = np.nonzero(pp["valid"] != 0)[0]
            lv = pp["level"][live]
            mnx, mny, mxx, mxy = (np.float32(v) for v in fr.bounds)
            grid = dict(min_x=mnx, min_y=mny, inv_w=np.float32(64) / np.float32(mxx - mnx), inv_h=np.float32(48) / np.float32(mxy - mny))
            om.WindowSearchGrid(fr.mvKeysUn, fr.mDescriptors, grid, pp["u"][live], pp["v"][live], np.float32(items[b]["th"]) * sf[lv], lv - 1,
                                lv + 1 - int(items[b]["kind"]), pp["desc"][live])
        lists.append((time.perf_counter() - t0) * 1e3)
    return stats(whole[1:]), stats(lists[1:])


def run(shape, params, B, repeats, percall, split):
    import torch
    from orb_slam3_modified_amd import ORBextractor
    from orb_slam3_modified_amd.matcher import ORBmatcher
    from orb_slam3_modified_amd.projmatch import ITEM_DTYPE, LDS_MAX, ProjMatchBatch, ProjMatchSide, lds_bytes, max_dist_reloc, max_dist_sim3
    H, W = shape
    ex = ORBextractor(*params, device_id=0)
    cap = ex.capacity
    x = Extracted(ex, B, H, W, repeats)
    s, dev = x.s, x.dev
    rng = np.random.default_rng(18)
    sf = np.asarray(ex.GetScaleFactors(), np.float32)
    bounds = np.array([[0, 0, W, H]] * B, np.float32)
    side = ProjMatchSide(x.kps, x.desc, x.counts, torch.from_numpy(bounds).to(dev), B, cap)
    pool = x.desc.view(-1, 32)
    om = ORBmatcher(ex, 0.9, True)
    res = {"frames": B, "capacity": cap, "keypoints_per_frame_median": int(np.median(x.hc[:, 0])), "d_extract_batch_device_ms": x.extract_ms,
           "lastmatch_r17_ms_256_items": LASTMATCH_R17_MS}
    libs = {"full": ProjMatchBatch(0)}
    if split:
        libs["nochain"] = ProjMatchBatch(0, library_path=timing_library_path("nochain", "ORBX_PROJMATCH_NO_CHAIN"))

    def timed(pb, args, out):
        ts = []
        for i in range(repeats + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            pb.search_device(*args, stream=s.cuda_stream, out=out)
            e1.record(s)
            e1.synchronize()
            if i >= 3:
                ts.append(e0.elapsed_time(e1))
        return stats(ts)

    def measure(name, items, pts, npts, taken, mcap):
        nb = len(items)
        t_items = torch.from_numpy(items.view(np.uint8).reshape(nb, 16)).to(dev)
        t_pts = torch.from_numpy(pts.view(np.uint8).reshape(nb, mcap, 32)).to(dev)
        t_npts = torch.from_numpy(npts).to(dev)
        t_taken = None if taken is None else torch.from_numpy(taken).to(dev)
        args = (side, t_items, t_pts, t_npts, pool, sf, t_taken, True)
        out = libs["full"].search_device(*args, stream=s.cuda_stream)
        torch.cuda.synchronize()
        got = out.nmatches.cpu().numpy(), out.kp_match.cpu().numpy()
        assert (got[0] >= 0).all()
        valid = np.array([int((pts[b, :npts[b]]["valid"] != 0).sum()) for b in range(nb)])
        r = {"items": nb, "mcap": mcap, "th": float(items[0]["th"]), "max_dist": float(items[0]["max_dist"]), "kind": int(items[0]["kind"]),
             "path": "lds" if lds_bytes(cap, mcap) + 4 * cap <= LDS_MAX else "global", "candidate_room": (LDS_MAX - lds_bytes(cap, mcap)) // 4,
             "valid_points_per_item_median": int(np.median(valid)), "matches_per_item_median": int(np.median(got[0])),
             "removed_by_rotation_per_item_median": int(np.median((got[1] == -2).sum(1)))}
        r["a_batched_device_call_ms"] = timed(libs["full"], args, out)
        a = r["a_batched_device_call_ms"]["median"]
        r["a_per_256_items_ms"] = round(a * 256 / nb, 4)
        r["a_per_256_items_over_lastmatch_r17"] = round(a * 256 / nb / LASTMATCH_R17_MS, 2)
        if split:
            o2 = libs["nochain"].search_device(*args, stream=s.cuda_stream)
            r["split_without_chain_ms"] = timed(libs["nochain"], args, o2)
            r["split_chain_share_of_a"] = round(1.0 - r["split_without_chain_ms"]["median"] / a, 3)
            r["a_again_after_the_split_ms"] = timed(libs["full"], args, out)     # the same build before and after the other one: the drift
        count = min(percall, nb)
        whole, lists = per_call(om, x, bounds, sf, items, pts, npts, taken, got, count)
        r["b_per_call_items_timed"] = count
        r["b_per_call_loop_ms"] = whole
        r["b_per_call_lists_only_ms"] = lists
        r["b_whole_loop_extrapolated_ms"] = round(whole["median"] * nb / count, 1)
        r["b_lists_only_extrapolated_ms"] = round(lists["median"] * nb / count, 1)
        r["b_lists_only_extrapolated_over_a"] = round(lists["median"] * nb / count / a, 1)
        res[name] = r
        return got

    # reloc: 2048 items, two runs
    frames = np.repeat(np.arange(B), 8)
    rows = [projected(rng, x.hk, x.hc, [((f - j) % B, 1.0 * j)], B, cap, cap) for f in range(B) for j in range(1, 9)]
    pts, npts = np.stack([r for r, _ in rows]), np.array([k for _, k in rows], np.int32)
    taken = (rng.random((len(frames), cap)) < 0.1).astype(np.uint8)
    items = np.array([(f, 0, 10.0, max_dist_reloc(100)) for f in frames], ITEM_DTYPE)
    got = measure("reloc_2048_items_th10_dist100", items, pts, npts, taken, cap)
    taken2 = taken | (got[1] >= 0).astype(np.uint8)
    items = np.array([(f, 0, 3.0, max_dist_reloc(64)) for f in frames], ITEM_DTYPE)
    measure("reloc_2048_items_th3_dist64_after_the_first", items, pts, npts, taken2, cap)
    del pts, rows
    # sim3: 256 items of ~2000 points
    mcap = 2 * cap
    rows = [projected(rng, x.hk, x.hc, [((f - 1) % B, 2.0), ((f - 2) % B, 4.0)], B, cap, mcap) for f in range(B)]
    pts, npts = np.stack([r for r, _ in rows]), np.array([k for _, k in rows], np.int32)
    items = np.array([(f, 1, 8.0, max_dist_sim3(1.5)) for f in range(B)], ITEM_DTYPE)
    measure("sim3_256_items_th8_ratio1.5", items, pts, npts, (rng.random((B, cap)) < 0.1).astype(np.uint8), mcap)
    for pb in libs.values():
        pb.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--percall", type=int, default=64)
    ap.add_argument("--no-split", action="store_true")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    assert args.repeats >= 9
    from orb_slam3_modified_amd import build
    out = {"stamp": build.stamp(), "repeats": args.repeats}
    out["euroc_752x480_1000"] = run((480, 752), (1000, 1.2, 8, 20, 7), args.frames, args.repeats, args.percall, not args.no_split)
    write_result(args.out, "tools/projmatch_times.py: batched relocalization and Sim3 SearchByProjection, HIP-event medians [min, max] of --repeats runs (ms); (b): wall clock", out)


if __name__ == "__main__":
    main()
