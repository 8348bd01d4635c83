"""Frame::ComputeStereoFishEyeMatches (src/Frame.cc:1126-1166) restated in numpy on the layouts of include/orbx_fisheye.h: what the batched
two-camera rig front-end (liborbx_fisheye.so) is held to.  The k-NN is oracle.pyoracle.knn2 (cv::BFMatcher(NORM_HAMMING).knnMatch(k = 2),
held to the reference elsewhere), the ratio test is evaluated with the reference's types, the finish loop is written out literally.
KannalaBrandt8::TriangulateMatches (:1156) is outside: its value arrives as `pair_depth`.  Nothing here needs a GPU."""
import numpy as np

from oracle import pyoracle as po

PAIR_DTYPE = np.dtype([("left", "<i4"), ("right", "<i4")])
EMPTY, MALFORMED = -1, -2


def ratio_accept(d0, d1):
    """(*it)[0].distance < (*it)[1].distance * 0.7 (:1151): DMatch::distance is a float, 0.7 a double literal -- the float is converted, the
    product is one double multiplication and the comparison is made in double."""
    a = np.asarray(d0).astype(np.float32).astype(np.float64)
    b = np.asarray(d1).astype(np.float32).astype(np.float64)
    return a < b * np.float64(0.7)


def frame_status(cL, cR, capL, capR):
    """0, or -1 (a count of -1: the extraction's overflow mark), or -2 (a count outside 0 .. capacity, a monoIndex outside 0 .. count)."""
    (nL, mL), (nR, mR) = (int(v) for v in cL), (int(v) for v in cR)
    if nL == -1 or nR == -1:
        return EMPTY
    if not (0 <= nL <= capL and 0 <= mL <= nL and 0 <= nR <= capR and 0 <= mR <= nR):
        return MALFORMED
    return 0


def match(descL, countsL, descR, countsR):
    """-> knn_idx, knn_dist [B, capL, 2], pairs [B, capL] (PAIR_DTYPE), npairs [B]."""
    B, capL, capR = descL.shape[0], descL.shape[1], descR.shape[1]
    knn_idx = np.full((B, capL, 2), -1, np.int32)
    knn_dist = np.full((B, capL, 2), 256, np.int32)
    pairs = np.zeros((B, capL), PAIR_DTYPE)
    pairs["left"], pairs["right"] = -1, -1
    npairs = np.zeros(B, np.int32)
    for f in range(B):
        st = frame_status(countsL[f], countsR[f], capL, capR)
        if st:
            npairs[f] = st
            continue
        (nL, monoLeft), (nR, monoRight) = (int(v) for v in countsL[f]), (int(v) for v in countsR[f])
        stereoDescLeft, stereoDescRight = descL[f, monoLeft:nL], descR[f, monoRight:nR]            # :1131-1132
        descMatches = 0
        if len(stereoDescLeft):
            idx, dist = po.knn2(stereoDescLeft, stereoDescRight)                                    # :1144
            for q in range(len(stereoDescLeft)):                                                    # :1150
                size = int((idx[q] >= 0).sum())
                for j in range(size):
                    knn_idx[f, monoLeft + q, j] = idx[q, j] + monoRight
                    knn_dist[f, monoLeft + q, j] = dist[q, j]
                if size >= 2 and ratio_accept(dist[q, 0], dist[q, 1]):                              # :1151
                    pairs[f, descMatches] = (q + monoLeft, idx[q, 0] + monoRight)
                    descMatches += 1
        npairs[f] = descMatches
    return knn_idx, knn_dist, pairs, npairs


def finish(pairs, npairs, pair_depth, countsL, countsR, capR):
    """-> l2r [B, capL], r2l [B, capR], depth [B, capL], nmatches [B]."""
    B, capL = pairs.shape
    l2r = np.full((B, capL), -1, np.int32)                                                          # :1134
    r2l = np.full((B, capR), -1, np.int32)                                                          # :1135
    depth = np.full((B, capL), -1.0, np.float32)                                                    # :1136
    nmatches = np.zeros(B, np.int32)
    for f in range(B):
        st = frame_status(countsL[f], countsR[f], capL, capR)
        n = int(npairs[f])
        if not st and n < 0:
            st = EMPTY if n == EMPTY else MALFORMED
        if not st and n > capL:
            st = MALFORMED
        if not st:
            Nleft, Nright = int(countsL[f, 0]), int(countsR[f, 0])
            p = pairs[f, :n]
            inside = (p["left"] >= 0) & (p["left"] < Nleft) & (p["right"] >= 0) & (p["right"] < Nright)
            if not inside.all() or (np.diff(p["left"].astype(np.int64)) <= 0).any():
                st = MALFORMED
        if st:
            nmatches[f] = st
            continue
        nMatches = 0
        for k in range(n):
            d = np.float32(pair_depth[f, k])
            if d > np.float32(0.0001):                                                              # :1157
                l2r[f, pairs[f, k]["left"]] = pairs[f, k]["right"]                                  # :1158
                r2l[f, pairs[f, k]["right"]] = pairs[f, k]["left"]                                  # :1159: the last one stays
                depth[f, pairs[f, k]["left"]] = d                                                   # :1161
                nMatches += 1
        nmatches[f] = nMatches
    return l2r, r2l, depth, nmatches
