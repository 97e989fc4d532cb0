"""Pure-numpy oracle of the new-map-point stage (uh_newpoints_*): Triangulate (src/basictypes/misc.cpp:923-1041), the distance-ratio /
octave-ratio check and the per-keypoint merge of MapManager (src/utils/mapmanager.cpp:10100-10700).

Float32 expressions keep the reference's written order; the products the reference takes through cv::Mat's operator* accumulate in
float64 and round once; A is formed in float32 and its null vector is np.linalg.svd of it in float64 (null="svd") or, as a second CPU
path, np.linalg.eigh of A^T A in float64 (null="eigh").  Next to every result the oracle returns, per match, the MARGIN: the smallest
relative distance of a tested quantity from its threshold over the checks the match went through.

Input format (shared with ucoslam_cv3_amd.newpoints.NewPoints.run):
  new_kf  dict(intr4 (4), scale_factors (L), pt (n, 2), octave (n), pose_g2f (4, 4), cam_center (3))
  pairs   list of dict(RT (4, 4), intr4, scale_factors, cam_center, pt, octave, matches (DMATCH_DTYPE: queryIdx = neighbour keypoint,
          trainIdx = new keyframe's keypoint))
"""
from __future__ import annotations

import numpy as np

f32 = np.float32
f64 = np.float64
DMATCH_DTYPE = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])

ACCEPTED, PARALLAX, W_ZERO, NOT_FINITE, DEPTH1, DEPTH2, CHI1, CHI2, ZERO_DIST, SCALE_RATIO = range(10)
MERGE_SMALLEST_OCTAVE, MERGE_LAST = 0, 1
NEAR = 1e-4             # a match whose smallest margin is below this is left out of the comparisons
MAX_NEAR_SHARE = 0.02   # ... and at most this share of a scene's matches may be


def ulp_diff(a, b):
    """distance in float32 representation steps (same-sign finite values)"""
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def _mm(a, b):
    """float GEMM the way OpenCV accumulates it: float64 sums, one rounding."""
    return (np.asarray(a, f64) @ np.asarray(b, f64)).astype(f32)


def projection_2(RT, intr4):
    fx, fy, cx, cy = [f32(v) for v in intr4]
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], f32)
    return _mm(K, np.asarray(RT, f32).reshape(4, 4)[:3, :])


def fundamental_12(intr_train, intr_query, RT):
    """getFund12 -> computeF12(eye, Ktrain, RT, Kquery) (framematcher.cpp:58-64, misc.cpp:893-920), the float chain."""
    RT = np.asarray(RT, f32).reshape(4, 4)
    R, t = RT[:3, :3], RT[:3, 3]
    R12 = R.T.copy()
    t12 = _mm(-R.T, t)

    def kinv(i4):
        fx, fy, cx, cy = [f64(f32(v)) for v in i4]
        return np.array([[1 / fx, 0, -cx / fx], [0, 1 / fy, -cy / fy], [0, 0, 1]], f64).astype(f32)

    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]], f32)
    return _mm(_mm(_mm(kinv(intr_train).T, tx), R12), kinv(intr_query))


def fundamental_12_f64(intr_train, intr_query, RT):
    """The same quantity from the same float inputs, every step in float64."""
    RT = np.asarray(RT, f32).reshape(4, 4).astype(f64)
    R, t = RT[:3, :3], RT[:3, 3]

    def K(i4):
        fx, fy, cx, cy = [f64(f32(v)) for v in i4]
        return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], f64)

    t12 = -R.T @ t
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]], f64)
    return np.linalg.inv(K(intr_train).T) @ tx @ R.T @ np.linalg.inv(K(intr_query))


def epipolar_line_sq_dist(kp1, kp2, F12):
    """misc.h:72-85, float."""
    F = np.asarray(F12, f32).reshape(3, 3)
    x1, y1, x2, y2 = f32(kp1[0]), f32(kp1[1]), f32(kp2[0]), f32(kp2[1])
    a = x1 * F[0, 0] + y1 * F[1, 0] + F[2, 0]
    b = x1 * F[0, 1] + y1 * F[1, 1] + F[2, 1]
    den = a * a + b * b
    if den == 0:
        return np.finfo(f32).max
    c = x1 * F[0, 2] + y1 * F[1, 2] + F[2, 2]
    num = a * x2 + b * y2 + c
    return num * num / den


def _null_vectors(A, null):
    """(n, 4) float64: the right singular vector of each float32 4x4 for its smallest singular value; NaN rows for non-finite A."""
    n = len(A)
    out = np.full((n, 4), np.nan, f64)
    ok = np.isfinite(A).all(axis=(1, 2))
    if ok.any():
        A64 = A[ok].astype(f64)
        if null == "svd":
            out[ok] = np.linalg.svd(A64)[2][:, 3, :]
        elif null == "eigh":
            out[ok] = np.linalg.eigh(np.swapaxes(A64, 1, 2) @ A64)[1][:, :, 0]
        else:
            raise ValueError(null)
    return out


def _norm3_as_float(d):
    d = d.astype(f64)
    return np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).astype(f32)


def _rel(q, thr, scale=None):
    """relative distance of q from thr; NaN (an undefined quantity decides nothing) counts as far away"""
    s = np.abs(f64(thr)) if scale is None else np.asarray(scale, f64)
    with np.errstate(all="ignore"):
        m = np.abs(np.asarray(q, f64) - f64(thr)) / s
    return np.where(np.isfinite(m), m, np.inf)


def triangulate_pair(new_kf, pair, max_chi2=5.998, ratio_factor=1.5 * 1.2, null="svd"):
    """Per match of one pair: xyz_cam (n, 3) float32 with NaN rows, xyz_global (n, 3), status (n) uint8, margin (n) float64."""
    m = np.asarray(pair["matches"])
    n = len(m)
    qi, ti = m["queryIdx"].astype(np.int64), m["trainIdx"].astype(np.int64)
    fx1, fy1, cx1, cy1 = [f32(v) for v in new_kf["intr4"]]
    fx2, fy2, cx2, cy2 = [f32(v) for v in pair["intr4"]]
    invfx1, invfy1, invfx2, invfy2 = f32(1) / fx1, f32(1) / fy1, f32(1) / fx2, f32(1) / fy2
    sf1, sf2 = np.asarray(new_kf["scale_factors"], f32), np.asarray(pair["scale_factors"], f32)
    inv1, inv2 = f32(1) / (sf1 * sf1), f32(1) / (sf2 * sf2)
    RT = np.asarray(pair["RT"], f32).reshape(4, 4)
    R, t = RT[:3, :3], RT[:3, 3]
    P2 = projection_2(RT, pair["intr4"])
    max_chi2, ratio_factor = f32(max_chi2), f32(ratio_factor)
    p1 = np.asarray(new_kf["pt"], f32).reshape(-1, 2)[ti]
    p2 = np.asarray(pair["pt"], f32).reshape(-1, 2)[qi]
    o1 = np.asarray(new_kf["octave"], np.int64)[ti]
    o2 = np.asarray(pair["octave"], np.int64)[qi]
    x1, y1, x2, y2 = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    one, zero = f32(1), f32(0)

    status = np.full(n, 255, np.uint8)
    margin = np.full(n, np.inf, f64)
    cam = np.full((n, 3), np.nan, f32)
    glob = np.full((n, 3), np.nan, f32)

    def refuse(cond, code):
        hit = (status == 255) & cond
        status[hit] = code

    def account(mg):   # a check's margin counts for every match that reaches the check
        live = status == 255
        margin[live] = np.minimum(margin[live], mg[live])

    with np.errstate(all="ignore"):
        # (a) misc.cpp:989-997
        xn1x, xn1y = (x1 - cx1) * invfx1, (y1 - cy1) * invfy1
        xn2x, xn2y = (x2 - cx2) * invfx2, (y2 - cy2) * invfy2
        i1 = (1.0 / np.sqrt(xn1x.astype(f64) ** 2 + xn1y.astype(f64) ** 2 + 1.0)).astype(f32)
        i2 = (1.0 / np.sqrt(xn2x.astype(f64) ** 2 + xn2y.astype(f64) ** 2 + 1.0)).astype(f32)
        r1 = np.stack([xn1x * i1, xn1y * i1, one * i1], 1)
        u = np.stack([xn2x * i2, xn2y * i2, one * i2], 1).astype(f64)
        R64 = R.astype(f64)
        r2 = np.stack([R64[0, k] * u[:, 0] + R64[1, k] * u[:, 1] + R64[2, k] * u[:, 2] for k in range(3)], 1).astype(f32)
        cos = (r1[:, 0] * r2[:, 0] + r1[:, 1] * r2[:, 1] + r1[:, 2] * r2[:, 2]).astype(f64)
        account(np.minimum(_rel(cos, 0.0, 1.0), _rel(cos, 0.9998)))
        refuse((cos < 0) | (cos > 0.9998), PARALLAX)
        # (b) :926-931
        A = np.empty((n, 4, 4), f32)
        A[:, 0, 0] = x1 * zero - fx1; A[:, 0, 1] = x1 * zero - zero; A[:, 0, 2] = x1 * one - cx1; A[:, 0, 3] = x1 * zero - zero
        A[:, 1, 0] = y1 * zero - zero; A[:, 1, 1] = y1 * zero - fy1; A[:, 1, 2] = y1 * one - cy1; A[:, 1, 3] = y1 * zero - zero
        for c in range(4):
            A[:, 2, c] = x2 * P2[2, c] - P2[0, c]
            A[:, 3, c] = y2 * P2[2, c] - P2[1, c]
        # (c) :933-938
        nv = _null_vectors(A, null)
        refuse(nv[:, 3] == 0, W_ZERO)
        X = (nv[:, :3] / nv[:, 3:4]).astype(f32)
        # (d) :1003
        refuse(~np.isfinite(X).all(axis=1), NOT_FINITE)
        # (e) :1007-1014
        Xn = np.sqrt((X.astype(f64) ** 2).sum(1))
        account(_rel(X[:, 2], 0.0, Xn))
        refuse(X[:, 2] <= 0, DEPTH1)
        X64 = X.astype(f64)
        X2 = np.stack([R64[k, 0] * X64[:, 0] + R64[k, 1] * X64[:, 1] + R64[k, 2] * X64[:, 2] + f64(t[k]) for k in range(3)], 1).astype(f32)
        X2n = np.sqrt((X2.astype(f64) ** 2).sum(1))
        account(_rel(X2[:, 2], 0.0, X2n))
        refuse(X2[:, 2] <= 0, DEPTH2)
        # (f) :1017-1022
        invZ1 = one / X[:, 2]
        qx, qy = fx1 * X[:, 0] * invZ1 + cx1, fy1 * X[:, 1] * invZ1 + cy1
        chi = inv1[o1] * ((qx - x1) * (qx - x1) + (qy - y1) * (qy - y1))
        account(_rel(chi, max_chi2))
        refuse(chi > max_chi2, CHI1)
        # (g) :1025-1031
        invZ2 = one / X2[:, 2]
        tx, ty = fx2 * X2[:, 0] * invZ2 + cx2, fy2 * X2[:, 1] * invZ2 + cy2
        chi = inv2[o2] * ((tx - x2) * (tx - x2) + (ty - y2) * (ty - y2))
        account(_rel(chi, max_chi2))
        refuse(chi > max_chi2, CHI2)
        tri_ok = status == 255
        cam[tri_ok] = X[tri_ok]
        # mapmanager.cpp:10139-10314
        T = np.asarray(new_kf["pose_g2f"], f32).reshape(4, 4)
        g = np.stack([T[k, 0] * X[:, 0] + T[k, 1] * X[:, 1] + T[k, 2] * X[:, 2] + T[k, 3] for k in range(3)], 1)
        c1, c2 = np.asarray(new_kf["cam_center"], f32), np.asarray(pair["cam_center"], f32)
        d1, d2 = _norm3_as_float(g - c1), _norm3_as_float(g - c2)
        refuse((d1 == 0) | (d2 == 0), ZERO_DIST)
        rd = d1 / d2
        ro = sf1[o1] / sf2[o2]
        lo, hi = rd * ratio_factor, ro * ratio_factor
        account(np.minimum(_rel(lo.astype(f64) - ro, 0.0, ro), _rel(rd.astype(f64) - hi, 0.0, hi)))
        refuse((lo < ro) | (rd > hi), SCALE_RATIO)
    acc = status == 255
    status[acc] = ACCEPTED
    glob[acc] = g[acc]
    return dict(xyz_cam=cam, xyz_global=glob, status=status, margin=margin)


def merge(new_kf, pairs, per_pair, merge_rule=MERGE_SMALLEST_OCTAVE):
    """The std::map keyed by trainIdx, filled in neighbour order then match order (mapmanager.cpp:10416-10479), and the choice per key
    (:10495-10696).  merge_rule: MERGE_SMALLEST_OCTAVE = the first candidate whose neighbour keypoint has the strictly smallest octave;
    MERGE_LAST = the last candidate (what :10604-10618 does as compiled: the running minimum is never assigned)."""
    cands = {}
    for j, (pair, r) in enumerate(zip(pairs, per_pair)):
        m = np.asarray(pair["matches"])
        for k in np.nonzero(r["status"] == ACCEPTED)[0]:
            cands.setdefault(int(m["trainIdx"][k]), []).append((j, int(k)))
    kp_idx, xyz, dist, cp, cm, obs_ptr, obs_pair, obs_kpt = [], [], [], [], [], [0], [], []
    for key in sorted(cands):
        lst = cands[key]
        best, best_oct = -1, np.iinfo(np.int32).max
        for i, (j, k) in enumerate(lst):
            o = int(np.asarray(pairs[j]["octave"])[pairs[j]["matches"]["queryIdx"][k]])
            if merge_rule == MERGE_LAST or o < best_oct:
                best, best_oct = i, o
        j, k = lst[best]
        kp_idx.append(key); xyz.append(per_pair[j]["xyz_global"][k]); dist.append(pairs[j]["matches"]["distance"][k]); cp.append(j); cm.append(k)
        obs_pair.append(-1); obs_kpt.append(key)
        for (jj, kk) in lst:
            obs_pair.append(jj); obs_kpt.append(int(pairs[jj]["matches"]["queryIdx"][kk]))
        obs_ptr.append(len(obs_pair))
    return dict(n_new=len(kp_idx), kp_idx=np.array(kp_idx, np.int32), xyz_global=np.array(xyz, f32).reshape(-1, 3),
                distance=np.array(dist, f32), chosen_pair=np.array(cp, np.int32), chosen_match=np.array(cm, np.int32),
                obs_ptr=np.array(obs_ptr, np.int32), obs_pair=np.array(obs_pair, np.int32), obs_kpt=np.array(obs_kpt, np.int32))


def run(new_kf, pairs, max_chi2=5.998, ratio_factor=1.5 * 1.2, null="svd", merge_rule=MERGE_SMALLEST_OCTAVE):
    """The mirror's dict (per-match arrays concatenated in pair order) plus margin (n_total) and match_xyz_global (n_total, 3)."""
    per = [triangulate_pair(new_kf, p, max_chi2, ratio_factor, null) for p in pairs]
    out = merge(new_kf, pairs, per, merge_rule)
    cat = lambda k, shape, dt: np.concatenate([r[k] for r in per]) if per else np.zeros(shape, dt)   # noqa: E731
    out.update(xyz_cam=cat("xyz_cam", (0, 3), f32), status=cat("status", (0,), np.uint8), margin=cat("margin", (0,), f64),
               match_xyz_global=cat("xyz_global", (0, 3), f32),
               pair_offset=np.cumsum([0] + [len(p["matches"]) for p in pairs]).astype(np.int64))
    return out
