"""What the timing tools of the side libraries share: the summary of a sample, a HIP-event timer, a batch of frames extracted into HBM and
the two pair lists of the pair matchers."""
from __future__ import annotations

import json
import os

import numpy as np


def stats(v):
    v = np.asarray(v, np.float64)
    return {"median": round(float(np.median(v)), 4), "min": round(float(v.min()), 4), "max": round(float(v.max()), 4), "n": int(len(v))}


def timed(stream, fn, n):
    """HIP events around fn() on `stream`: n runs after three warm-up runs."""
    import torch
    ts = []
    for i in range(n + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        if i >= 3:
            ts.append(e0.elapsed_time(e1))
    return stats(ts)


class Extracted:
    """B synthetic H x W frames extracted into HBM on a stream of their own (kps, desc, counts: torch tensors), the extraction's time
    (`extract_ms`) and the host copies (hk, hd, hc)."""

    def __init__(self, ex, B, H, W, repeats):
        import torch
        from orb_slam3_modified_amd import synth
        from orb_slam3_modified_amd._lib import KP_DTYPE
        self.B, self.cap, self.dev = B, ex.capacity, torch.device("cuda:0")
        self.s = torch.cuda.Stream(device=self.dev)
        t = torch.from_numpy(synth.make_stream(B, H, W)).to(self.dev)
        z = lambda *shape, dt=torch.uint8: torch.zeros(shape, dtype=dt, device=self.dev)   # noqa: E731
        self.kps, self.desc, self.counts = z(B, self.cap, 28), z(B, self.cap, 32), z(B, 2, dt=torch.int32)
        p = lambda x: x.data_ptr()   # noqa: E731
        torch.cuda.synchronize()
        self.extract_ms = timed(self.s, lambda: ex.extract_batch_device(p(t), B, H, W, W, H * W, p(self.kps), p(self.desc), p(self.counts), (0, 1000),
                                                                        stream=self.s.cuda_stream), repeats)
        self.hk = self.kps.cpu().numpy().view(KP_DTYPE).reshape(B, self.cap)
        self.hd, self.hc = self.desc.cpu().numpy(), self.counts.cpu().numpy()


def pair_lists(B):
    """256 pairs (f, f + 1) and 2560 pairs (every frame against the ten that follow it), frame indices modulo B."""
    return {"256_pairs_f_f1": np.array([(f, (f + 1) % B) for f in range(B)], np.int32),
            "2560_pairs_f_ten_others": np.array([(f, (f + j) % B) for f in range(B) for j in range(1, 11)], np.int32)}


def write_result(path, header, out):
    """The result as one JSON line on stdout and, under a `# header` line, indented in `path`."""
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("# " + header + "\n" + json.dumps(out, indent=1) + "\n")
    print("wrote", path)
