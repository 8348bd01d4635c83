"""A plain sequential statement of include/orbx_rigbow.h: the stacked rig frame and both modes of the rig SearchByBoW, written from the
description of the loop (src/ORBmatcher.cc:223-425 with F.Nleft != -1, :765-905 with NLeft != -1), with a trace of what every query saw.
What the GPU suite holds liborbx_rigbow.so to.

FeatureVectors are dicts node -> list of stacked feature indices (the list order is the scan order).  nleft = -1: a single-camera frame."""
from __future__ import annotations

import numpy as np

from tests.match_batch_model import rotation_bin, three_maxima

FRAME, KEYFRAMES = 0, 1
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
_F = np.float32


def stack(kps_l, desc_l, counts_l, kps_r, desc_r, counts_r, cap_s):
    """(kps_s [F, cap_s], desc_s [F, cap_s, 32], counts_s [F, 2], nleft [F]) of F rig frames; a malformed frame gives zero rows, {-1, 0}
    and -1."""
    F, cap_l, cap_r = len(desc_l), desc_l.shape[1], desc_r.shape[1]
    kps_s, desc_s = np.zeros((F, cap_s), kps_l.dtype), np.zeros((F, cap_s, 32), np.uint8)
    counts_s, nleft = np.zeros((F, 2), np.int32), np.zeros(F, np.int32)
    for f in range(F):
        nl, nr = int(counts_l[f][0]), int(counts_r[f][0])
        if not (0 <= nl <= cap_l and 0 <= nr <= cap_r and nl + nr <= cap_s):
            counts_s[f, 0], nleft[f] = -1, -1
            continue
        kps_s[f, :nl], kps_s[f, nl:nl + nr] = kps_l[f, :nl], kps_r[f, :nr]
        desc_s[f, :nl], desc_s[f, nl:nl + nr] = desc_l[f, :nl], desc_r[f, :nr]
        counts_s[f, 0], nleft[f] = nl + nr, nl
    return kps_s, desc_s, counts_s, nleft


def search_by_bow(desc_a, angle_a, valid_a, fv_a, nleft_a, desc_b, angle_b, valid_b, fv_b, nleft_b, mode=FRAME, nn_ratio=0.7,
                  check_orientation=True, trace=None):
    """(nmatches, b2a [len(desc_b)], a2b [len(desc_a), 2]).  valid_a / valid_b: uint8 arrays or None (all valid); valid_b only counts in
    keyframes mode.  `trace`, a list, receives one dict per query that ran: node, a, best1, idx, best2, best1r, idxr, best2r (what the
    reference's dead variable would hold), skipped (taken slots it passed over), left / right (the slots it bound, or -1); and at the end
    one dict {"removed": [slots the rotation filter cleared], "bins": the 30 sizes}."""
    desc_a, desc_b = np.asarray(desc_a, np.uint8).reshape(-1, 32), np.asarray(desc_b, np.uint8).reshape(-1, 32)
    na, nb = len(desc_a), len(desc_b)
    b2a = np.full(nb, -1, np.int64)
    kf = mode == KEYFRAMES
    bins = [[] for _ in range(30)]
    nmatches = 0
    for node in sorted(set(fv_a) & set(fv_b)):
        for ia in fv_a[node]:
            if kf and nleft_a != -1 and ia >= nleft_a:                       # :800
                continue
            if valid_a is not None and not valid_a[ia]:
                continue
            best1, idx, best2, best1r, idxr, best2r, skipped = 256, -1, 256, 256, -1, 256, []
            for ib in fv_b[node]:
                if kf:
                    if nleft_b != -1 and ib >= nleft_b:                      # :820
                        continue
                    if valid_b is not None and not valid_b[ib]:
                        continue
                if b2a[ib] >= 0:
                    skipped.append(int(ib))
                    continue
                dist = int(_POP[desc_a[ia] ^ desc_b[ib]].sum())
                if kf or nleft_b == -1 or ib < nleft_b:
                    if dist < best1:
                        best2, best1, idx = best1, dist, int(ib)
                    elif dist < best2:
                        best2 = dist
                else:
                    if dist < best1r:
                        best2r, best1r, idxr = best1r, dist, int(ib)
                    elif dist < best2r:
                        best2r = dist
            left = right = -1
            if best1 <= (49 if kf else 50):
                if _F(best1) < _F(nn_ratio) * _F(best2):
                    left = idx
                if not kf and best1r <= 50:                                  # `|| true`: no ratio test
                    right = idxr
            for slot in (left, right):
                if slot >= 0:
                    b2a[slot] = ia
                    nmatches += 1
                    if check_orientation:
                        b = rotation_bin(angle_a[ia], angle_b[slot])
                        if 0 <= b < 30:
                            bins[b].append(slot)
            if trace is not None:
                trace.append(dict(node=node, a=int(ia), best1=best1, idx=idx, best2=best2, best1r=best1r, idxr=idxr, best2r=best2r,
                                  skipped=skipped, left=left, right=right))
    removed = []
    if check_orientation:
        keep = three_maxima([len(b) for b in bins])
        for i, members in enumerate(bins):
            if i not in keep:
                for slot in members:
                    b2a[slot] = -1
                    nmatches -= 1
                    removed.append(slot)
    if trace is not None:
        trace.append(dict(removed=removed, bins=[len(b) for b in bins]))
    a2b = np.full((na, 2), -1, np.int32)
    split = nb + 1 if (kf or nleft_b == -1) else nleft_b
    for slot in np.nonzero(b2a >= 0)[0]:
        a2b[b2a[slot], int(slot >= split)] = slot
    assert nmatches == int((b2a >= 0).sum())
    return nmatches, b2a.astype(np.int32), a2b


def malformed(counts_a, fv_n_a, fv_feat_a, nleft_a, ok_a, counts_b, fv_n_b, fv_feat_b, nleft_b, ok_b):
    """Whether the header calls the pair malformed: ok_* = the frame index is inside its batch; fv_feat_* = the entries the lists use."""
    if not (ok_a and ok_b):
        return True
    for c, k, feat, nl in ((counts_a, fv_n_a, fv_feat_a, nleft_a), (counts_b, fv_n_b, fv_feat_b, nleft_b)):
        if c < 0 or k < 0 or not -1 <= nl <= c or any(int(v) >= c for v in feat):
            return True
    return False
