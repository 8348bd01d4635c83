#!/usr/bin/env python3
"""Projection-front times (liborbx_project.so) -> profiles/project_times_r22.txt.

A synthetic map at the EuRoC shape (752 x 480, 8 levels at 1.2): 256 keyframes with a pose each and 1000 map points each, placed where the
keyframe sees them (depth 1 .. 8 m, the normal along the viewing ray, the distance range so that the predicted level is a drawn octave);
the table of 256 000 points is resident in HBM.  Three shapes:
  last    256 items x 906 slots: frame f projects 900 points of keyframe f - 1 (TrackWithMotionModel), 6 slots skipped
  reloc   2048 items x 906 slots: frame f projects the points of 8 candidate keyframes (Relocalization)
  fuse    5120 items x 2012 slots, ~1000 of them listed: keyframe f's points into each of its 20 neighbours (SearchInNeighbors, the shape of
          tools/fuse_times.py's own_into_neighbours: qcap = the extractor's capacity)
For each: (a) the device call, HIP events on one stream, `--repeats` runs after three warm-up runs: median [min, max]; the bytes the
algorithm needs over the median give the achieved rate and its share of the 8.0 TB/s HBM peak.  (b) the host twin over the same items on
one core (wall clock); (a)'s rows are checked against its rows in the same run.  (c) the host-to-device copy of exactly the rows (a) makes
unnecessary, from pinned memory (HIP events) and from pageable memory (wall clock).  Nothing about speed is asserted; the file records
whether the fuse call takes less time than the upload it replaces, and the ratio.
"""
from __future__ import annotations

import argparse
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from times_util import stats, timed, write_result  # noqa: E402
OUT = os.path.join(ROOT, "profiles", "project_times_r22.txt")
HBM_PEAK = 8.0e12
W, H, NLEVELS, PER = 752, 480, 8, 1000
NEIGHBOURS = [d for d in range(-10, 11) if d]


def source_hash() -> str:
    """sha256 over the library's kernel source and its header, first 16 hex digits."""
    import hashlib
    from orb_slam3_modified_amd import build
    h = hashlib.sha256()
    for f in (os.path.join(build.CSRC, build.PROJECT_SOURCE), os.path.join(ROOT, "include", "orbx_project.h")):
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def world(rng, K):
    """(table, obs, items [K], octave [K * PER], angle [K * PER]): the map and a pose per keyframe."""
    from orb_slam3_modified_amd.project import ITEM_DTYPE, TABLE_DTYPE
    F = np.float32
    fx, fy, cx, cy, mbf = 458.654, 457.296, 367.215, 248.375, 47.90639
    table, obs = np.zeros(K * PER, TABLE_DTYPE), rng.integers(1, 9, K * PER).astype(np.int32)
    items = np.zeros(K, ITEM_DTYPE)
    octave = rng.choice(NLEVELS, K * PER, p=[0.3, 0.22, 0.16, 0.12, 0.08, 0.06, 0.04, 0.02]).astype(np.int32)
    angle = (rng.random(K * PER) * 360).astype(F)
    for f in range(K):
        axis = np.array([0.2 * np.sin(0.7 * f), 1.0, 0.1 * np.cos(0.3 * f)])
        axis /= np.linalg.norm(axis)
        a = 0.004 * f
        x, y, z = axis * np.sin(a / 2)
        w = np.cos(a / 2)
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        t = np.array([0.01 * f, -0.02, 0.1 + 0.005 * f])
        Ow = -(R.T @ t)
        items[f]["Rcw"], items[f]["tcw"], items[f]["Ow"], items[f]["q"] = R.astype(F).ravel(), t.astype(F), Ow.astype(F), np.array([x, y, z, w], F)
        items[f]["fx"], items[f]["fy"], items[f]["cx"], items[f]["cy"], items[f]["mbf"] = fx, fy, cx, cy, mbf
        items[f]["bounds"], items[f]["th"] = (0, 0, W, H), 3.0
        rows = slice(f * PER, (f + 1) * PER)
        depth = 1 + 7 * rng.random(PER)
        Pc = np.stack([(rng.random(PER) * W - cx) * depth / fx, (rng.random(PER) * H - cy) * depth / fy, depth], 1)
        P = (Pc - t) @ R
        PO = P - Ow
        dist = np.linalg.norm(PO, axis=1)
        maxd = (dist * 1.2 ** octave[rows] * 0.95).astype(F)
        table["pos"][rows], table["normal"][rows] = P.astype(F), (PO / dist[:, None]).astype(F)
        table["min_inv"][rows], table["max_inv"][rows], table["max_dist"][rows] = F(0.8) * (maxd / F(4.3)), F(1.2) * maxd, maxd
    return table, obs, items, octave, angle


def lists(rng, kind, K, items, octave, angle):
    """(items of the call, slots or idx, nslots) of one shape."""
    from orb_slam3_modified_amd.project import SLOT_DTYPE
    if kind == "fuse":
        pairs = [(f, (f + d) % K) for f in range(K) for d in NEIGHBOURS]
        mcap = 2012
        idx = np.full((len(pairs), mcap), -1, np.int32)
        for p, (f, k) in enumerate(pairs):
            idx[p, :PER] = f * PER + np.arange(PER)
        idx[:, 7:PER:97] = -1                                                  # already in the keyframe: skipped
        return items[[k for _, k in pairs]], idx, np.full(len(pairs), PER, np.int32)
    pairs = [(f, (f - 1) % K) for f in range(K)] if kind == "last" else [(f, (f + 3 * c + 2) % K) for f in range(K) for c in range(8)]
    mcap = 906
    slots = np.zeros((len(pairs), mcap), SLOT_DTYPE)
    for p, (f, k) in enumerate(pairs):
        pts = k * PER + rng.permutation(PER)[:mcap]
        slots["point"][p], slots["octave"][p], slots["angle"][p] = pts, octave[pts], angle[pts]
    slots["point"][:, 11::151] = -1                                            # outliers, points already found: skipped
    return items[[f for f, _ in pairs]], slots, np.full(len(pairs), mcap, np.int32)


def run(kind, K, repeats, table, obs, items, octave, angle, t_table, t_obs, s, dev, lsf, sf):
    import torch
    from orb_slam3_modified_amd import project as pj
    rng = np.random.default_rng(22)
    its, slots, nslots = lists(rng, kind, K, items, octave, angle)
    B, mcap = slots.shape
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (-1,)) if a.dtype.names else np.ascontiguousarray(a)).to(dev)  # noqa: E731
    t_items, t_slots, t_n = up(its), up(slots), up(nslots)
    pb = pj.ProjectBatch(0)
    call = {"last": lambda **kw: pb.last(t_table, t_obs, t_items, t_slots, t_n, stream=s.cuda_stream, **kw),
            "reloc": lambda **kw: pb.reloc(t_table, t_items, t_slots, t_n, lsf, NLEVELS, stream=s.cuda_stream, **kw),
            "fuse": lambda **kw: pb.fuse(t_table, t_items, t_slots, t_n, lsf, sf, stream=s.cuda_stream, **kw)}[kind]
    twin = {"last": lambda: pj.reference_last(table, obs, its, slots, nslots),
            "reloc": lambda: pj.reference_reloc(table, its, slots, nslots, lsf, NLEVELS),
            "fuse": lambda: pj.reference_fuse(table, its, slots, nslots, lsf, sf)}[kind]
    out = call()
    s.synchronize()
    res = {"items": B, "mcap": mcap, "rot_kind": "MATRIX", "sum_order": "LTR", "log_kind": "DOUBLE"}
    res["a_device_ms"] = timed(s, lambda: call(out=out), repeats)
    torch.cuda.synchronize()
    got = out.host()
    point = slots if kind == "fuse" else slots["point"]
    live = int(((point >= 0) & (np.arange(mcap)[None] < nslots[:, None])).sum())
    valid = int(got.nvalid.sum())
    # a slot, its row; of a listed point's record what the emitter fetches (last: the position's 16 bytes, and obs for a valid row)
    nbytes = B * mcap * 32 + int(nslots.sum()) * (4 if kind == "fuse" else 16) + (live * 16 + valid * 4 if kind == "last" else live * 36)
    res["rows"], res["listed_points"], res["valid_rows"], res["algorithm_bytes"] = B * mcap, live, valid, nbytes
    res["a_achieved_TB_per_s"] = round(nbytes / (res["a_device_ms"]["median"] * 1e-3) / 1e12, 3)
    res["a_share_of_hbm_peak_8TBps"] = round(res["a_achieved_TB_per_s"] * 1e12 / HBM_PEAK, 3)
    ts = []
    for rep in range(3):
        t0 = time.perf_counter()
        ref = twin()
        ts.append((time.perf_counter() - t0) * 1e3)
    assert ref.rows.tobytes() == got.rows.tobytes() and np.array_equal(ref.nvalid, got.nvalid), "device rows != host twin rows"
    res["b_host_twin_one_core_ms"] = stats(ts[1:])
    res["b_over_a"] = round(res["b_host_twin_one_core_ms"]["median"] / res["a_device_ms"]["median"], 1)
    rows_pageable = torch.from_numpy(ref.rows.view(np.uint8).reshape(B, mcap, 32))
    rows_pinned = rows_pageable.pin_memory()
    dst = torch.empty((B, mcap, 32), dtype=torch.uint8, device=dev)
    res["rows_bytes"] = int(dst.numel())

    def copy_from(host):
        with torch.cuda.stream(s):
            dst.copy_(host, non_blocking=True)
    res["c_h2d_rows_pinned_ms"] = timed(s, lambda: copy_from(rows_pinned), repeats)
    ts = []
    for i in range(repeats + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dst.copy_(rows_pageable)
        torch.cuda.synchronize()
        if i >= 3:
            ts.append((time.perf_counter() - t0) * 1e3)
    res["c_h2d_rows_pageable_wall_ms"] = stats(ts)
    res["c_pinned_over_a"] = round(res["c_h2d_rows_pinned_ms"]["median"] / res["a_device_ms"]["median"], 1)
    res["a_slowest_below_c_pinned_fastest"] = bool(res["a_device_ms"]["max"] < res["c_h2d_rows_pinned_ms"]["min"])
    pb.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    import torch
    from orb_slam3_modified_amd import build
    stamp = build.stamp()
    stamp["project_source_hash"] = source_hash()
    out = {"stamp": stamp, "repeats": args.repeats, "keyframes": args.keyframes, "npoints": args.keyframes * PER, "nlevels": NLEVELS}
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    sf = np.ones(NLEVELS, np.float32)
    for i in range(1, NLEVELS):
        sf[i] = np.float32(sf[i - 1] * np.float32(1.2))
    lsf = float(np.float32(math.log(float(sf[1]))))                           # mfLogScaleFactor = log(1.2f), stored in a float
    table, obs, items, octave, angle = world(np.random.default_rng(2222), args.keyframes)
    t_table = torch.from_numpy(table.view(np.uint8).reshape(len(table), 48)).to(dev)
    t_obs = torch.from_numpy(obs).to(dev)
    for kind in ("last", "reloc", "fuse"):
        out[kind] = run(kind, args.keyframes, args.repeats, table, obs, items, octave, angle, t_table, t_obs, s, dev, lsf, sf)
    out["fuse_call_below_the_upload_it_replaces"] = out["fuse"]["a_slowest_below_c_pinned_fastest"]
    write_result(args.out, "tools/project_times.py: the LastFrame, relocalization and Fuse projection fronts, HIP-event medians [min, max] of --repeats "
                 "runs (ms); (b) and the pageable copy: wall clock", out)


if __name__ == "__main__":
    main()
