#!/usr/bin/env python3
"""Batched ComputeDistinctiveDescriptors times (liborbx_mpdesc.so) -> profiles/mpdesc_times_r13.txt.

256 synthetic frames at the EuRoC shape (752 x 480; 1000 features, 1.2, 8 levels, 20 / 7) resident in HBM as keyframes -- the side of
profiles/fuse_times_r12.txt.  Every keyframe owns `--points` map points (300).  The expected load is a guess from the reference's
structure, not a measurement: a point's N is drawn from
    70 %  2 .. 8      25 %  9 .. 30      4.5 %  31 .. 64      0.45 %  65 .. 256      0.05 %  257 .. 1024
and its observations are rows drawn at random from the owner and the keyframes that follow it (one row a keyframe, wrapping modulo 256;
above 256 observations a keyframe is visited again).  Per batch, HIP events around orbx_mpdesc_select_device, `--repeats` runs after three
warm-up runs, median [min, max]:
  (t) the whole batch under the default routing
  (f) per form: the batch's small (N <= 64), mid (65 .. 256) and large (> 256) points as batches of their own, and a batch of empty
      points -- the four launches' fixed cost, which every (f) figure contains
  (h) a single-core host loop of the same specification written for this tool (C++: the N x N matrix, std::sort of every row, the
      element at (int)(0.5 * (N - 1)), strict <), compiled with g++ -O2 at run time; wall clock, results compared with (t)'s
  (b) the routing boundaries, the one sweep that decides a default: batches of 16 384 points (1024 above N = 64) of one N each, every form that can take
      that N forced by ORBX_MPDESC_SMALL_MAX / ORBX_MPDESC_MID_MAX; and the whole batch under moved boundaries
Beside them the extraction of the same run and, read from profiles/fuse_times_r12.txt, the FeatureVector transform and the Fuse searches.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from times_util import Extracted, stats, timed, write_result  # noqa: E402
OUT = os.path.join(ROOT, "profiles", "mpdesc_times_r13.txt")
FUSE_TIMES = os.path.join(ROOT, "profiles", "fuse_times_r12.txt")
DISTRIBUTION = ((0.70, 2, 8), (0.25, 9, 30), (0.045, 31, 64), (0.0045, 65, 256), (0.0005, 257, 1024))

HOST_LOOP = r"""
#include <algorithm>
#include <climits>
#include <cstdint>
#include <vector>
// src/MapPoint.cc:369-397 on the ABI's arrays; every observation is valid
extern "C" void host_select(const uint8_t* desc, int cap, const int32_t* obs, const int32_t* start, int npoints, int32_t* best, int32_t* median) {
  std::vector<int> D, v;
  for (int m = 0; m < npoints; m++) {
    const int s = start[m], N = start[m + 1] - s;
    if (N == 0) { best[m] = median[m] = -1; continue; }
    D.assign((size_t)N * N, 0);
    for (int i = 0; i < N; i++)
      for (int j = i + 1; j < N; j++) {
        const uint64_t* a = (const uint64_t*)(desc + ((size_t)obs[2 * (s + i)] * cap + obs[2 * (s + i) + 1]) * 32);
        const uint64_t* b = (const uint64_t*)(desc + ((size_t)obs[2 * (s + j)] * cap + obs[2 * (s + j) + 1]) * 32);
        int d = 0;
        for (int k = 0; k < 4; k++) d += __builtin_popcountll(a[k] ^ b[k]);
        D[(size_t)i * N + j] = d; D[(size_t)j * N + i] = d;
      }
    int BestMedian = INT_MAX, BestIdx = 0;
    for (int i = 0; i < N; i++) {
      v.assign(D.begin() + (size_t)i * N, D.begin() + (size_t)(i + 1) * N);
      std::sort(v.begin(), v.end());
      const int med = v[(int)(0.5 * (N - 1))];
      if (med < BestMedian) { BestMedian = med; BestIdx = i; }
    }
    best[m] = BestIdx; median[m] = BestMedian;
  }
}
"""


def draw_sizes(rng, n):
    u = rng.random(n)
    out = np.zeros(n, np.int64)
    lo = 0.0
    for share, a, b in DISTRIBUTION:
        sel = (u >= lo) & (u < lo + share)
        out[sel] = rng.integers(a, b + 1, int(sel.sum()))
        lo += share
    out[out == 0] = 2
    return out


def observations(rng, hc, owner, sizes):
    """CSR observations: point m of keyframe owner[m] is seen in the sizes[m] keyframes from its owner on, one random row each."""
    from orb_slam3_modified_amd.mpdesc import OBS_DTYPE
    B = len(hc)
    start = np.zeros(len(sizes) + 1, np.int32)
    start[1:] = np.cumsum(sizes)
    obs = np.zeros(int(start[-1]), OBS_DTYPE)
    which = np.arange(len(obs)) - np.repeat(start[:-1], sizes)
    obs["frame"] = (np.repeat(owner, sizes) + which) % B
    obs["row"] = (rng.random(len(obs)) * hc[obs["frame"], 0]).astype(np.int32)
    return obs, start


def host_loop():
    if shutil.which("g++") is None:
        return None
    d = tempfile.mkdtemp(prefix="mpdesc_host_")
    src, lib = os.path.join(d, "host.cpp"), os.path.join(d, "host.so")
    open(src, "w").write(HOST_LOOP)
    subprocess.check_call(["g++", "-O2", "-mpopcnt", "-shared", "-fPIC", "-o", lib, src])
    L = C.CDLL(lib)
    L.host_select.restype = None
    L.host_select.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return L


class Job:
    """One batch on the device and a call of a handle on it."""

    def __init__(self, x, side, obs, start):
        import torch
        self.x, self.side, self.M = x, side, len(start) - 1
        self.obs = torch.from_numpy(obs.view(np.int32).reshape(-1, 2).copy()).to(x.dev)
        self.start = torch.from_numpy(start).to(x.dev)
        self.table = torch.zeros((self.M, 32), dtype=torch.uint8, device=x.dev)
        self.best = torch.zeros(self.M, dtype=torch.int32, device=x.dev)
        self.median = torch.zeros(self.M, dtype=torch.int32, device=x.dev)
        torch.cuda.synchronize()

    def call(self, db):
        return db.select_device(self.side, self.obs, self.start, None, self.table, stream=self.x.s.cuda_stream, best=self.best, median=self.median)

    def time(self, db, repeats):
        self.call(db)
        return timed(self.x.s, lambda: self.call(db), repeats)


def handle(small_max=None, mid_max=None):
    from orb_slam3_modified_amd.mpdesc import DistinctBatch
    for name, v in (("ORBX_MPDESC_SMALL_MAX", small_max), ("ORBX_MPDESC_MID_MAX", mid_max)):
        if v is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = str(v)
    db = DistinctBatch(0)
    os.environ.pop("ORBX_MPDESC_SMALL_MAX", None)
    os.environ.pop("ORBX_MPDESC_MID_MAX", None)
    return db


def run(B, repeats, per_frame, sweep_points):
    import torch
    from orb_slam3_modified_amd import ORBextractor
    from orb_slam3_modified_amd.mpdesc import MID_CAP, MID_MAX, SMALL_CAP, SMALL_MAX, DistinctSide
    H, W, params = 480, 752, (1000, 1.2, 8, 20, 7)
    ex = ORBextractor(*params, device_id=0)
    x = Extracted(ex, B, H, W, repeats)
    cap = x.cap
    res = {"frames": B, "capacity": cap, "points_per_keyframe": per_frame, "distribution": [list(d) for d in DISTRIBUTION],
           "routing": {"small_max": SMALL_MAX, "mid_max": MID_MAX}, "d_extract_batch_device_ms": x.extract_ms}
    rng = np.random.default_rng(329)
    M = B * per_frame
    sizes, owner = draw_sizes(rng, M), np.repeat(np.arange(B), per_frame)
    obs, start = observations(rng, x.hc, owner, sizes)
    res["points"], res["observations"] = M, int(len(obs))
    res["n_percentiles_50_90_99_max"] = [int(v) for v in np.percentile(sizes, (50, 90, 99, 100))]
    side = DistinctSide(x.desc, x.counts, B, cap)
    db = handle()
    # (t)
    whole = Job(x, side, obs, start)
    res["t_whole_batch_ms"] = whole.time(db, repeats)
    torch.cuda.synchronize()
    best, median = whole.best.cpu().numpy(), whole.median.cpu().numpy()
    assert (best >= 0).all()
    res["t_us_per_point"] = round(1000.0 * res["t_whole_batch_ms"]["median"] / M, 5)
    # (f)
    classes = {"small": sizes <= SMALL_MAX, "mid": (sizes > SMALL_MAX) & (sizes <= MID_MAX), "large": sizes > MID_MAX}
    for name, sel in classes.items():
        o, s = observations(rng, x.hc, owner[sel], sizes[sel])
        r = res.setdefault("f_" + name, {"points": int(sel.sum()), "observations": int(len(o))})
        if sel.sum():
            r["ms"] = Job(x, side, o, s).time(db, repeats)
    empty = Job(x, side, obs[:1], np.zeros(M + 1, np.int32))
    res["f_empty_points_fixed_cost_ms"] = empty.time(db, repeats)
    # (h)
    L = host_loop()
    if L is not None:
        hb, hm = np.zeros(M, np.int32), np.zeros(M, np.int32)
        flat = np.ascontiguousarray(obs.view(np.int32))
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            L.host_select(x.hd.ctypes.data, cap, flat.ctypes.data, start.ctypes.data, M, hb.ctypes.data, hm.ctypes.data)
            ts.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(hb, best) and np.array_equal(hm, median)
        res["h_host_loop_ms"] = stats(ts)
        res["h_us_per_point"] = round(1000.0 * res["h_host_loop_ms"]["median"] / M, 4)
        res["h_over_t"] = round(res["h_host_loop_ms"]["median"] / res["t_whole_batch_ms"]["median"], 1)
        res["results_equal_host_loop"] = True
    # (b) one N a batch, every form that can take it
    forms = {"small": (SMALL_CAP, MID_CAP), "mid": (0, MID_CAP), "large": (0, 0)}
    hs = {name: handle(*b) for name, b in forms.items()}
    sweep = res.setdefault("b_one_n_ms", {"points": sweep_points})
    for n in (2, 4, 8, 16, 24, 32, 48, 64, 96, 128, 192, 256, 384):
        pts = sweep_points if n <= 64 else sweep_points // 16
        o, s = observations(rng, x.hc, rng.integers(0, B, pts), np.full(pts, n))
        job = Job(x, side, o, s)
        row = sweep.setdefault("n_%d" % n, {"points": pts})
        ref = None
        for name, (cap_n) in (("small", SMALL_CAP), ("mid", MID_CAP), ("large", 1024)):
            if n <= cap_n:
                row[name] = job.time(hs[name], repeats)["median"]
                torch.cuda.synchronize()
                got = (job.best.cpu().numpy(), job.median.cpu().numpy(), job.table.cpu().numpy())
                assert ref is None or all(np.array_equal(a, b) for a, b in zip(ref, got)), (n, name)
                ref = got
        row["fastest"] = min((k for k in row if k not in ("points", "fastest")), key=lambda k: row[k])
    for h in hs.values():
        h.close()
    moved = res.setdefault("b_whole_batch_moved_boundaries_ms", {})
    for sm, mm_ in ((8, 256), (16, 256), (32, 256), (48, 256), (64, 256), (64, 128), (64, 64), (32, 128)):
        h = handle(sm, mm_)
        moved["small_max_%d_mid_max_%d" % (sm, mm_)] = whole.time(h, repeats)["median"]
        h.close()
    db.close()
    # beside the feeding stages and the Fuse searches
    if os.path.exists(FUSE_TIMES):
        ft = json.loads(open(FUSE_TIMES).read().split("\n", 1)[1])["euroc_752x480_1000"]
        fuse = ft["g_grids_device_ms"]["median"] + ft["own_into_neighbours"]["s_search_device_ms"]["median"] + ft["neighbours_into_own"]["s_search_device_ms"]["median"]
        feed = x.extract_ms["median"] + ft["d_transform_featurevectors_ms"]["median"]
        res["beside"] = {"extract_this_run_ms": x.extract_ms["median"], "transform_fuse_times_r12_ms": ft["d_transform_featurevectors_ms"]["median"],
                         "fuse_grids_and_both_searches_fuse_times_r12_ms": round(fuse, 4),
                         "select_per_keyframe_us": round(1000.0 * res["t_whole_batch_ms"]["median"] / B, 3),
                         "extraction_plus_transform_per_keyframe_us": round(1000.0 * feed / B, 3), "fuse_per_keyframe_us": round(1000.0 * fuse / B, 3),
                         "select_over_extraction_plus_transform": round(res["t_whole_batch_ms"]["median"] / feed, 4)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--points", type=int, default=300, help="map points a keyframe owns")
    ap.add_argument("--sweep-points", type=int, default=16384, help="points of a one-N batch of the boundary sweep")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    assert args.repeats >= 10
    from orb_slam3_modified_amd import build
    out = {"stamp": build.stamp(), "repeats": args.repeats}
    out["euroc_752x480_1000"] = run(args.frames, args.repeats, args.points, args.sweep_points)
    write_result(args.out, "tools/mpdesc_times.py: batched ComputeDistinctiveDescriptors, HIP-event medians [min, max] of --repeats runs (ms)", out)


if __name__ == "__main__":
    main()
