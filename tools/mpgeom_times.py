#!/usr/bin/env python3
"""Batched MapPoint::UpdateNormalAndDepth times (liborbx_mpgeom.so) -> profiles/mpgeom_times_r26.txt.

256 synthetic frames at the EuRoC shape (752 x 480; 1000 features, 1.2, 8 levels, 20 / 7) resident in HBM as keyframes, `--points` map
points (20 000) whose observation counts are drawn as tests/mpdesc_cases.random_observations draws them (N uniform in 0 .. 40, one point of
70 and one of 300 observations).  Camera centres and positions are drawn; the octaves are the extraction's.  Per batch, HIP events around
orbx_mpgeom_update_device, `--repeats` runs after three warm-up runs, median [min, max]:
  (t) the whole batch under the default routing, for each (sum_order, div_kind)
  (r) the same batch with ORBX_MPGEOM_SMALL_MAX forced to 0, 8, 16, 32, 64: the routing boundary
  (e) a batch of empty points: the three launches' fixed cost
and, measured in the same run, what the call replaces:
  (a) the library's host twin (orbx_mpgeom_update_reference) on one core, wall clock, results compared with (t)'s
  (b) the upload of the 48-byte rows (hipMemcpyAsync from pinned memory, HIP events)
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from times_util import Extracted, stats, timed, write_result  # noqa: E402
OUT = os.path.join(ROOT, "profiles", "mpgeom_times_r26.txt")


def handle(small_max=None):
    from orb_slam3_modified_amd.mpgeom import NormalDepthBatch
    if small_max is not None:
        os.environ["ORBX_MPGEOM_SMALL_MAX"] = str(small_max)
    nb = NormalDepthBatch(0)
    os.environ.pop("ORBX_MPGEOM_SMALL_MAX", None)
    return nb


def run(B, repeats, M):
    import torch
    from orb_slam3_modified_amd import ORBextractor, mpgeom
    from orb_slam3_modified_amd.frustum import TABLE_DTYPE
    from orb_slam3_modified_amd.mpgeom import OBS_DTYPE, NormalDepthSide
    sys.path.insert(0, ROOT)
    from tests.mpdesc_cases import random_observations
    H, W, params = 480, 752, (1000, 1.2, 8, 20, 7)
    ex = ORBextractor(*params, device_id=0)
    x = Extracted(ex, B, H, W, repeats)
    cap = x.cap
    sf = np.asarray(ex.GetScaleFactors(), np.float32)
    rng = np.random.default_rng(426)
    obs, start = random_observations(x.hc, M, 426)
    sizes = np.diff(start)
    ref = np.zeros(M, OBS_DTYPE)
    first = np.minimum(start[:-1], len(obs) - 1)
    ref["frame"], ref["row"] = obs["frame"][first], obs["row"][first]          # mpRefKF: the first observer
    centres = np.zeros((B, 8), np.float32)
    centres[:, :3] = rng.uniform(-5, 5, (B, 3))
    table = np.zeros(M, TABLE_DTYPE)
    table["pos"] = (rng.uniform(6, 14, (M, 3)) * rng.choice([-1, 1], (M, 3))).astype(np.float32)
    res = {"frames": B, "capacity": cap, "points": M, "observations": int(len(obs)),
           "n_percentiles_50_90_99_max": [int(v) for v in np.percentile(sizes, (50, 90, 99, 100))], "routing": {"small_max": mpgeom.SMALL_MAX},
           "d_extract_batch_device_ms": x.extract_ms}
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(x.dev)   # noqa: E731
    side = NormalDepthSide(x.kps, x.counts, t(centres), B, cap)
    d_obs, d_start, d_ref = t(obs.view(np.int32).reshape(-1, 2)), t(start), t(ref.view(np.int32).reshape(-1, 2))
    d_table = t(table.view(np.uint8).reshape(M, 48))
    d_n, d_min = torch.zeros(M, dtype=torch.int32, device=x.dev), torch.zeros(M, dtype=torch.float32, device=x.dev)
    torch.cuda.synchronize()

    def call(nb, order=0, kind=0, starts=d_start):
        return nb.update_device(side, d_obs, starts, d_ref, d_table, sf, None, order, kind, stream=x.s.cuda_stream, n=d_n, min_dist=d_min)

    nb = handle()
    # (t) and (a)
    hside = NormalDepthSide(x.hk, x.hc, centres, B, cap)
    for order, kind, name in ((0, 0, "ltr_quotient"), (0, 1, "ltr_reciprocal"), (1, 0, "tree_quotient"), (1, 1, "tree_reciprocal")):
        res["t_whole_batch_%s_ms" % name] = timed(x.s, lambda: call(nb, order, kind), repeats)
        torch.cuda.synchronize()
        got = (d_n.cpu().numpy(), d_min.cpu().numpy(), d_table.cpu().numpy().view(np.uint32))
        want_table = table.copy()
        ts = []
        for _ in range(3):
            want_table[:] = table
            t0 = time.perf_counter()
            want = mpgeom.reference(hside, obs, start, ref, want_table, sf, None, order, kind)
            ts.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(got[0], want.n) and np.array_equal(got[1].view(np.uint32), want.min_dist.view(np.uint32))
        assert np.array_equal(got[2].reshape(-1), want_table.view(np.uint32).reshape(-1))
        res["a_host_twin_one_core_%s_ms" % name] = stats(ts)
    res["results_equal_host_twin"] = True
    med = res["t_whole_batch_ltr_quotient_ms"]["median"]
    res["t_us_per_point"] = round(1000.0 * med / M, 5)
    res["a_over_t"] = round(res["a_host_twin_one_core_ltr_quotient_ms"]["median"] / med, 1)
    # (r)
    moved = res.setdefault("r_small_max_ms", {})
    for sm in (0, 8, 16, 32, 64):
        h = handle(sm)
        moved["small_max_%d" % sm] = timed(x.s, lambda: call(h), repeats)
        h.close()
    # (e)
    res["e_empty_points_fixed_cost_ms"] = timed(x.s, lambda: call(nb, starts=torch.zeros_like(d_start)), repeats)
    # (b)
    pinned = torch.from_numpy(table.view(np.uint8).reshape(M, 48).copy()).pin_memory()
    with torch.cuda.stream(x.s):
        res["b_upload_48_byte_rows_ms"] = timed(x.s, lambda: d_table.copy_(pinned, non_blocking=True), repeats)
    res["b_over_t"] = round(res["b_upload_48_byte_rows_ms"]["median"] / med, 2)
    nb.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    assert args.repeats >= 10
    from orb_slam3_modified_amd import build
    out = {"stamp": build.stamp(), "repeats": args.repeats}
    out["euroc_752x480_1000"] = run(args.frames, args.repeats, args.points)
    write_result(args.out, "tools/mpgeom_times.py: batched UpdateNormalAndDepth, HIP-event medians [min, max] of --repeats runs (ms)", out)


if __name__ == "__main__":
    main()
