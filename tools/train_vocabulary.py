#!/usr/bin/env python3
"""Train a DBoW2 vocabulary on the GPU (ORBVocabulary.create = TemplatedVocabulary::create after SeedRandOnce(seed)).

Images: .npy (2-D uint8) or binary PGM (P5) files, or --synthetic N frames of the project's synthetic stream.  Each frame is extracted with
the batch extractor and is one document, as Frame::ComputeBoW sees it.  Writes the reference's text format (OUT.txt) and the exact binary
cache (OUT.bin) and prints the stats.

  python tools/train_vocabulary.py OUT [IMAGES...] [--synthetic N] [-k 10] [-L 6] [--weighting 0] [--scoring 0] [--seed 0]
                                       [--nfeatures 1000] [--device-min-node -1]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def read_image(path: str) -> np.ndarray:
    if path.endswith(".npy"):
        img = np.load(path)
    else:
        b = open(path, "rb").read()
        tok, pos = [], 0
        while len(tok) < 4:   # "P5 width height maxval" with comments
            while b[pos:pos + 1].isspace():
                pos += 1
            if b[pos:pos + 1] == b"#":
                pos = b.index(b"\n", pos) + 1
                continue
            end = pos
            while not b[end:end + 1].isspace():
                end += 1
            tok.append(b[pos:end])
            pos = end
        if tok[0] != b"P5" or int(tok[3]) > 255:
            raise ValueError(f"{path}: only 8-bit binary PGM (P5) is read")
        w, h = int(tok[1]), int(tok[2])
        img = np.frombuffer(b, np.uint8, w * h, pos + 1).reshape(h, w)
    if img.dtype != np.uint8 or img.ndim != 2:
        raise ValueError(f"{path}: a 2-D uint8 image is needed")
    return np.ascontiguousarray(img)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("images", nargs="*")
    ap.add_argument("--synthetic", type=int, default=0)
    ap.add_argument("-k", type=int, default=10)
    ap.add_argument("-L", type=int, default=6)
    ap.add_argument("--weighting", type=int, default=0, help="0 TF_IDF, 1 TF, 2 IDF, 3 BINARY")
    ap.add_argument("--scoring", type=int, default=0, help="0 L1_NORM .. 5 DOT_PRODUCT")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--nfeatures", type=int, default=1000)
    ap.add_argument("--device-min-node", type=int, default=-1)
    a = ap.parse_args()
    from orb_slam3_modified_amd import ORBextractor, ORBVocabulary, synth
    ex = ORBextractor(a.nfeatures, 1.2, 8, 20, 7, device_id=0)
    docs = []
    groups = {}
    for p in a.images:   # the batch extractor takes frames of one shape at a time
        img = read_image(p)
        groups.setdefault(img.shape, []).append(img)
    for a0 in range(0, a.synthetic, 64):
        groups.setdefault(("synthetic", a0), []).extend(synth.make_stream(min(64, a.synthetic - a0), 480, 640, 9000 + a0))
    for imgs in groups.values():
        for b in range(0, len(imgs), 64):
            docs += [r[2] for r in ex.extract_batch(np.stack(imgs[b:b + 64]), (0, 1000))]
    if not docs:
        ap.error("no images")
    v = ORBVocabulary(ex)
    st = v.create(docs, a.k, a.L, a.weighting, a.scoring, seed=a.seed, device_min_node=a.device_min_node)
    v.saveToTextFile(a.out + ".txt")
    v.saveBinary(a.out + ".bin")
    print(f"{len(docs)} documents, {sum(len(d) for d in docs)} descriptors -> {v.info()}")
    print(st)


if __name__ == "__main__":
    main()
