"""The constructed inputs of vocabulary training's large-node tests (tests/test_voc_train_model.py on the CPU, tests/test_gpu_voc_train.py on
the GPU): five descriptor sets, each the smallest that takes csrc/train/orbx_train.hip into one of its second regimes, generated
procedurally (no descriptor array is committed).  tools/make_voc_train_golden.py --large records the reference's create on them in
tests/golden/voc_train_large.npz.  Nothing here needs a GPU."""
import hashlib

import numpy as np

BLOCK = 256          # kBlock: descriptors per workgroup
CHUNK = 65536        # blocks per k_seed_select chunk * BLOCK, and the IDF descent's chunk
TF_IDF, TF, IDF = 0, 1, 2
HOST_ONLY = 2 ** 31 - 1


def clustered(n, ncentres, flip, seed):
    """n near-duplicates around ncentres random centres: every bit of a centre flips with probability `flip`."""
    rng = np.random.default_rng(seed)
    centres = rng.integers(0, 256, (ncentres, 32), dtype=np.uint8)
    pick = rng.integers(0, ncentres, n)
    out = np.empty((n, 32), np.uint8)
    for a in range(0, n, 16384):      # row chunks draw the same stream as one (n, 256) call
        p = pick[a:a + 16384]
        flips = rng.random((len(p), 256)) < flip
        out[a:a + len(p)] = np.packbits(np.unpackbits(centres[p], axis=1) ^ flips, axis=1)
    return out


def edge_positions(n):
    """The first and the last element of every block of 256, ascending."""
    p = np.arange(n)
    return p[(p % BLOCK == 0) | (p % BLOCK == BLOCK - 1)]


def edges(n, others, seed):
    """One descriptor A everywhere except at the block edges, which cycle through `others` further distinct random descriptors."""
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 256, (others + 1, 32), dtype=np.uint8)
    assert len({r.tobytes() for r in d}) == others + 1
    out = np.repeat(d[:1], n, axis=0)
    pos = edge_positions(n)
    out[pos] = d[1 + np.arange(len(pos)) % others]
    return out


GENERATORS = {"clustered": clustered, "edges": edges}

# name -> generator, its arguments, k, L, weighting, scoring, seed of rand(), document offsets, the in-between device_min_node.
# Offsets: 5 to 9 uneven documents, one of them empty, no boundary on a multiple of 256 or 65536; where N allows, small documents wholly
# past descriptor 65536, so that a word's Ni depends on the second descent chunk.  The clustered sets have many more centres than k * k:
# with fewer, two seeds of a level-2 node share a centre, their means coincide, one cluster empties and the reference does not complete.
# `mid`: the root and the larger children on the device, the smaller children (still above k) in the host loop.
CASES = {
    # kc * nb = 16 * 64 = 1024: k_scan_excl with per = 1 and every thread busy
    "scan_1024": dict(gen="clustered", args=(16384, 800, 0.03, 1024), k=16, L=2, weighting=TF, scoring=0, seed=31,
                      offsets=(0, 3001, 3001, 9000, 9077, 16384), mid=1000),
    # kc * nb = 16 * 65 = 1040: per = 2, threads 520.. idle (b0 == b1 == m), the last block holds one row
    "scan_1040": dict(gen="clustered", args=(16385, 800, 0.03, 1040), k=16, L=2, weighting=TF_IDF, scoring=0, seed=32,
                      offsets=(0, 2999, 3050, 3050, 9001, 9013, 16385), mid=1000),
    # 258 blocks: k_seed_select carries one chunk; every pick is a block's first or last element; the seeding stops at 7 centres
    "edges_66k": dict(gen="edges", args=(66001, 6, 66), k=10, L=2, weighting=IDF, scoring=0, seed=25,
                      offsets=(0, 130, 130, 30001, 65601, 65700, 65795, 66001), mid=1000),
    # 274 blocks (two chunks), kc * nb = 5480 (per = 6), the IDF descent in two chunks
    "chunks_70k": dict(gen="clustered", args=(70001, 1500, 0.03, 70), k=20, L=2, weighting=TF_IDF, scoring=0, seed=33,
                       offsets=(0, 20011, 20011, 20040, 65700, 65743, 66950, 69990, 70001), mid=3500),
    # 1026 blocks: k_bitcount's 1024 workgroups take a second round, a full tile and one of 77 rows; five chunks of seeding and descent
    "stride_262k": dict(gen="clustered", args=(1024 * 256 + 256 + 77, 60, 0.03, 262), k=5, L=2, weighting=IDF, scoring=0, seed=36,
                        offsets=(0, 50, 70003, 70003, 131100, 131130, 200001, 262300, 262477), mid=50000),
}
IDF_CASES = tuple(n for n, c in CASES.items() if c["weighting"] in (TF_IDF, IDF))
DEFAULT_CASE = "chunks_70k"      # the one trained at device_min_node = -1 (4096)
DEFAULT_MIN_NODE = 4096          # ORBX_TRAIN_DEVICE_MIN_NODE


def generate(name):
    """-> (desc (n, 32) uint8, offsets int64)."""
    c = CASES[name]
    desc = np.ascontiguousarray(GENERATORS[c["gen"]](*c["args"]))
    off = np.array(c["offsets"], np.int64)
    assert off[0] == 0 and off[-1] == len(desc) and np.all(np.diff(off) >= 0)
    return desc, off


def digest(desc, off):
    return hashlib.sha256(desc.tobytes() + np.asarray(off, np.int64).tobytes()).hexdigest()


def split(trace, k, thr):
    """(device nodes, host nodes) of orbx_train_vocabulary at device_min_node = thr, from the model's trace (one entry per k-means node in
    depth-first order): a node runs on the device when it has at least max(thr, k + 1) descriptors and its parent ran there."""
    thr = max(thr, k + 1)
    dev = host = 0
    on_dev = {}                   # level -> whether the last node seen at that level ran on the device
    for t in trace:
        d = t["n"] >= thr and (t["level"] == 1 or on_dev[t["level"] - 1])
        on_dev[t["level"]] = d
        dev, host = dev + d, host + (not d)
    return dev, host
