"""numpy restatement of FrameExtractor::processStereo steps 3-7 and process_rgbd (src/utils/frameextractor.cpp from :1419, read after macro
expansion) for kptImageScaleFactor == 1: plain loops, float32 / float64 scalars where the C types are float / double, std::round as half away
from zero, cvRound as half to even.  Written from the reference text, not from the library's stereo_math.hpp.

Two places where the reference reads out of bounds or throws are decided here as the library documents them:
  * a left keypoint whose rounded row is outside [0, rows) has no candidates (the reference indexes its vector of buckets unchecked);
  * the SAD offsets stop where the shifted 6 x 6 window still lies inside the right image (the reference throws from cv::Mat::operator()).
A right keypoint whose rounded row is outside the image lands in NO bucket: the reference's loop runs from max(0, r) to min(rows - 1, r),
which is empty then."""
import math

import numpy as np

KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
DBL_MAX = np.finfo(np.float64).max
FLT_MAX = float(np.finfo(np.float32).max)


def std_round(v) -> int:
    """int(std::round(v)) for a float or double v given as a float32 / float64 scalar: halves away from zero (|v| + 0.5 is exact in double
    for every float32 the tests use)."""
    v = float(v)
    return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


def cv_round(v) -> int:
    """cvRound(float): nearest, halves to even."""
    return int(np.rint(np.float32(v)))


def _as_ints(desc):
    return [int.from_bytes(bytes(row), "little") for row in np.asarray(desc, np.uint8).reshape(-1, 32)]


def hamming(a: int, b: int) -> int:
    return bin(a ^ b).count("1")


def stereo_depth(L, R, lk, ld, rk, rd, bl, fx, max_desc_dist):
    """-> (depth float32 (n_left), match int32 (n_left))."""
    L, R = np.asarray(L), np.asarray(R)
    rows, cols = L.shape
    assert R.shape == L.shape
    nl, nr = len(lk), len(rk)
    ldi, rdi = _as_ints(ld), _as_ints(rd)
    mdd = np.float32(max_desc_dist)
    buckets = [[] for _ in range(rows)]
    for j in range(nr):
        sh = 0.0
        y = float(rk["y"][j])   # double y = pt.y
        lo = max(0, std_round(y - sh))
        hi = min(rows - 1, std_round(y + sh))
        for r in range(lo, hi + 1):
            buckets[r].append(j)
    depth = np.zeros(nl, np.float32)
    match = np.full(nl, -1, np.int32)
    blfx = np.float32(bl) * np.float32(fx)   # float * float
    for i in range(nl):
        lux, luy, loct = np.float32(lk["x"][i]), np.float32(lk["y"][i]), int(lk["octave"][i])
        r = std_round(luy)
        if r < 0 or r >= rows:   # (deviation: unchecked index in the reference)
            continue
        best, best_d = -1, DBL_MAX
        for j in buckets[r]:
            if np.float32(rk["x"][j]) > lux or abs(int(rk["octave"][j]) - loct) > 1:
                continue
            d = np.float32(hamming(ldi[i], rdi[j]))
            if d < mdd:
                if float(d) < best_d:
                    best_d, best = float(d), j
        match[i] = best
        if best == -1:
            continue
        hw = 7 // 2
        lx, ly = std_round(lux), std_round(luy)
        if lx < hw or lx + hw >= cols or ly < hw or ly + hw >= rows:
            continue
        rpx, rpy = np.float32(rk["x"][best]), np.float32(rk["y"][best])
        rx, ry = std_round(rpx), std_round(rpy)
        if rx < hw or rx + hw >= cols or ry < hw or ry + hw >= rows:
            continue
        wl = L[ly - hw:ly + hw, lx - hw:lx + hw].astype(np.int64)
        o_lo, o_hi = max(-7, -rx), min(7, cols - 1 - rx)
        o_lo, o_hi = max(o_lo, hw - rx), min(o_hi, cols - hw - rx)   # (deviation: the reference throws outside this range)
        cost = [0.0] * 15
        best_c, b = DBL_MAX, -1
        for o in range(o_lo, o_hi + 1):
            c = rx + o
            wr = R[ry - hw:ry + hw, c - hw:c + hw].astype(np.int64)
            s = float(np.abs(wl - wr).sum())
            if s < best_c:
                best_c, b = s, o + 7
            cost[o + 7] = s
        if b > o_lo + 7 and b < o_hi + 7:
            c0, c1, c2 = np.float64(cost[b - 1]), np.float64(cost[b]), np.float64(cost[b + 1])
            with np.errstate(divide="ignore", invalid="ignore"):
                delta = np.float64(0.5) * (c0 - c2) / (c0 + c2 - np.float64(2) * c1) + np.float64(b) - np.float64(7)
                xr = np.float64(rpx) + delta
                depth[i] = np.float32(np.float64(blfx) / (np.float64(lux) - xr))
    return depth, match


def brute_force_matches(L, lk, ld, rk, rd, max_desc_dist):
    """The match alone, formulated without buckets: among ALL right keypoints whose rounded row equals the left keypoint's, after the x and
    octave filters and the distance bound, the minimum over (distance, j) keys."""
    rows = np.asarray(L).shape[0]
    ldi, rdi = _as_ints(ld), _as_ints(rd)
    rrow = np.array([std_round(np.float32(y)) for y in rk["y"]], np.int64) if len(rk) else np.zeros(0, np.int64)
    out = np.full(len(lk), -1, np.int32)
    for i in range(len(lk)):
        r = std_round(np.float32(lk["y"][i]))
        if r < 0 or r >= rows:
            continue
        keys = [(hamming(ldi[i], rdi[j]), int(j)) for j in np.nonzero(rrow == r)[0]
                if not (np.float32(rk["x"][j]) > np.float32(lk["x"][i])) and abs(int(rk["octave"][j]) - int(lk["octave"][i])) <= 1]
        keys = [k for k in keys if np.float32(k[0]) < np.float32(max_desc_dist)]
        if keys:
            out[i] = min(keys)[1]
    return out


def rgbd_depth(kpts, D, depth_scale):
    """process_rgbd: depth[i] = D.at<uint16_t>(Point(kpts[i].pt)) * rgb_depthscale (int * float, in float) where non-zero; the library gives 0
    for a pixel outside the depth image (the reference reads unchecked)."""
    D = np.asarray(D)
    out = np.zeros(len(kpts), np.float32)
    for i in range(len(kpts)):
        x, y = cv_round(kpts["x"][i]), cv_round(kpts["y"][i])
        if x < 0 or x >= D.shape[1] or y < 0 or y >= D.shape[0]:
            continue
        v = int(D[y, x])
        if v != 0:
            out[i] = np.float32(v) * np.float32(depth_scale)
    return out
