"""numpy oracle of PnPSolver::solvePnPRansac (src/optimization/pnpsolver.cpp:36-114) as include/ucoslam_hip.h specifies it.

The three-point problem is solved by a route that is numerically different from csrc/p3p_math.hpp: the same cosine-rule equations,
but with the roles of the points rotated (the unknown of the quartic is s1 / s2 where the kernel's is s3 / s1), the polynomial
multiplied out by np.polymul, its roots taken from the companion matrix (np.roots) where the kernel uses Ferrari's closed form, the
three distances refined by Newton with a general linear solve (where the kernel takes two steps with the adjugate written out), and
the pose from an SVD alignment (Kabsch) where the kernel builds two orthonormal frames.  Both are judged by the 60-digit solve of
tests/golden/p3p_golden.npz (tests/test_p3p_branches_host.py).  Every solution can be checked on its own
(check_solution).  The fourth-point pick is in double; the matrix construction and the inlier test are float32 in the written order.
"""
from __future__ import annotations

import numpy as np

f32, f64 = np.float32, np.float64
MAX_ERR = f32(5.99)
NEAR = 1e-4              # relative band around a threshold inside which a (hypothesis, match) pair is not compared
MAX_NEAR_SHARE = 0.02    # at most this share of a scene's pairs may lie in the band
MAX_ILL_SHARE = 0.10     # at most this share of a scene's hypotheses may be ill-conditioned
JITTER, JITTER_MOVE = 1e-12, 1e-9
IMAG_TOL = 1e-10
COLLINEAR_SIN2 = 1e-16


def _bearings(intr4, px):
    fx, fy, cx, cy = [float(v) for v in intr4]
    xn = np.stack([(px[:, 0] - cx) / fx, (px[:, 1] - cy) / fy, np.ones(len(px))], 1)
    return xn / np.linalg.norm(xn, axis=1, keepdims=True), xn


def _kabsch(P, C):
    pm, cm = P.mean(0), C.mean(0)
    Hm = (P - pm).T @ (C - cm)
    U, _, Vt = np.linalg.svd(Hm)
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    return R, cm - R @ pm


def _refine_distances(s, j, P):
    """Newton on the three cosine-rule equations |s_a j_a - s_b j_b|^2 = |P_a - P_b|^2 in the three distances (np.linalg.solve on the
    3 x 3 Jacobian, until the step no longer shrinks): u = N / D carries the quartic root's error magnified by 1 / D, and without this
    the oracle was up to 3.3e-5 off a 60-digit solve on well-separated roots (tests/golden/make_p3p_golden.py)."""
    pairs = ((0, 1), (0, 2), (1, 2))
    d2 = np.array([(P[a] - P[b]) @ (P[a] - P[b]) for a, b in pairs])
    cs = np.array([j[a] @ j[b] for a, b in pairs])
    last = np.inf
    for _ in range(6):
        f = np.array([s[a] ** 2 + s[b] ** 2 - 2 * s[a] * s[b] * c for (a, b), c in zip(pairs, cs)]) - d2
        J = np.zeros((3, 3))
        for r, ((a, b), c) in enumerate(zip(pairs, cs)):
            J[r, a], J[r, b] = 2 * (s[a] - s[b] * c), 2 * (s[b] - s[a] * c)
        with np.errstate(all="ignore"):
            try:
                step = np.linalg.solve(J, f)
            except np.linalg.LinAlgError:
                break
        size = np.abs(step).max()
        if not np.isfinite(size) or size >= last:
            break
        s, last = s - step, size
    return s


def p3p(intr4, P, px):
    """P (4, 3), px (4, 2) in float64.  Returns (solutions, chosen, err4): solutions = list of dict(R, t, s (3 distances)) in ascending
    s3 / s1; chosen = index of the smallest fourth-point error (lowest index on ties), -1 = the iteration is skipped."""
    P, px = np.asarray(P, f64), np.asarray(px, f64)
    j, xn = _bearings(intr4, px)
    e1, e2 = P[1] - P[0], P[2] - P[0]
    cr = np.cross(e1, e2)
    if not np.isfinite(P).all() or not np.isfinite(px).all() or not (cr @ cr > COLLINEAR_SIN2 * (e1 @ e1) * (e2 @ e2)) or not ((P[2] - P[1]) @ (P[2] - P[1]) > 0):
        return [], -1, np.zeros(0)
    # roles rotated: A = point 2, B = point 3, C = point 1
    o = (1, 2, 0)
    A, B, Cc = P[o[0]], P[o[1]], P[o[2]]
    jA, jB, jC = j[o[0]], j[o[1]], j[o[2]]
    a2, b2, c2 = (B - Cc) @ (B - Cc), (A - Cc) @ (A - Cc), (A - B) @ (A - B)
    ca, cb, cg = jB @ jC, jA @ jC, jA @ jB
    k, q = (a2 - c2) / b2, c2 / b2
    N = np.array([k - 1, -2 * k * cb, k + 1])
    D = np.array([-2 * ca, 2 * cg])
    Wp = np.array([-q, 2 * q * cb, 1 - q])
    poly = np.polyadd(np.polyadd(np.polymul(N, N), np.polymul(np.polymul(D, D), Wp)), -2 * cg * np.polymul(N, D))
    if not np.isfinite(poly).all() or poly[0] == 0:
        return [], -1, np.zeros(0)
    sols = []
    for r in np.roots(poly):
        if abs(r.imag) > IMAG_TOL * (1 + abs(r.real)):
            continue
        v = r.real
        for _ in range(2):
            dv = np.polyval(np.polyder(poly), v)
            if dv != 0:
                v = v - np.polyval(poly, v) / dv
        u = np.polyval(N, v) / np.polyval(D, v)
        den = 1 + v * v - 2 * v * cb
        if not (v > 0 and u > 0 and den > 0 and np.isfinite(u)):
            continue
        sA = np.sqrt(b2 / den)
        s = np.zeros(3)
        s[o[0]], s[o[1]], s[o[2]] = sA, u * sA, v * sA
        s = _refine_distances(s, j[:3], P[:3])
        if not (s > 0).all():
            continue
        R, t = _kabsch(P[:3], s[:, None] * j[:3])
        if not (np.isfinite(R).all() and np.isfinite(t).all()):
            continue
        sols.append(dict(R=R, t=t, s=s))
    sols.sort(key=lambda d: d["s"][2] / d["s"][0])
    err = np.zeros(len(sols))
    for i, d in enumerate(sols):
        with np.errstate(all="ignore"):
            Xc = d["R"] @ P[3] + d["t"]
            err[i] = (Xc[0] / Xc[2] - xn[3, 0]) ** 2 + (Xc[1] / Xc[2] - xn[3, 1]) ** 2
    chosen, best = -1, np.inf
    for i, e in enumerate(err):
        if e < best:
            best, chosen = e, i
    return sols, chosen, err


def check_solution(intr4, P, px, sol):
    """The largest violation of: R'R = I, det R = +1, the three sample points reproject onto their pixels (normalised coordinates),
    positive point distances.  inf when a distance is not positive."""
    R, t, s = sol["R"], sol["t"], sol["s"]
    if not (s > 0).all():
        return np.inf
    _, xn = _bearings(intr4, np.asarray(px, f64))
    Xc = np.asarray(P, f64)[:3] @ R.T + t
    rep = np.abs(Xc[:, :2] / Xc[:, 2:3] - xn[:3, :2]).max()
    dist = np.abs(np.linalg.norm(Xc, axis=1) - s).max()
    return max(np.abs(R.T @ R - np.eye(3)).max(), abs(np.linalg.det(R) - 1), rep, dist)


def rodrigues_vec(R):
    """Rotation matrix -> vector by another route than the kernel's: theta from the trace (arccos), the axis as the eigenvector of R for
    the eigenvalue 1, its sign from the skew part."""
    c = min(1.0, max(-1.0, 0.5 * (np.trace(R) - 1)))
    sk = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = 0.5 * np.linalg.norm(sk)
    theta = np.arctan2(s, c) if (s < 1e-3 or c < -0.999) else np.arccos(c)
    if s < 1e-7 and c > 0:
        return 0.5 * sk
    w, V = np.linalg.eig(R)
    ax = np.real(V[:, np.argmin(np.abs(w - 1))])
    ax /= np.linalg.norm(ax)
    if s >= 1e-13:   # the skew part (absolute error 1e-16) still says which of a, -a it is; below 1e-7 this was taken for pi itself,
        if ax @ sk < 0:   # which cost up to 1e-7 on R at pi - 1e-8 (tests/test_p3p_branches_host.py, family rot)
            ax = -ax
    else:   # theta = pi: the sign convention of the near-pi branch (first non-tiny component positive, as the diagonal form gives)
        big = np.argmax(np.abs(ax) > 1e-6)
        if ax[big] < 0:
            ax = -ax
    return ax * theta


def se3_set(rt6):
    """Se3Transform::set(const float*), se3transform.h:143-176: float32 in the written order; cos / sin in double on the float angle."""
    rx, ry, rz, tx, ty, tz = [f32(v) for v in rt6]
    nsqa = rx * rx + ry * ry + rz * rz
    a = f32(np.sqrt(nsqa))
    i_a = f32(1.0 / f64(a)) if a else f32(0)
    rnx, rny, rnz = rx * i_a, ry * i_a, rz * i_a
    cos_a, sin_a = f32(np.cos(f64(a))), f32(np.sin(f64(a)))
    omc = f32(1.0 - f64(cos_a))
    M = np.zeros(12, f32)
    M[0] = cos_a + rnx * rnx * omc
    M[1] = rnx * rny * omc - rnz * sin_a
    M[2] = rny * sin_a + rnx * rnz * omc
    M[3] = tx
    M[4] = rnz * sin_a + rnx * rny * omc
    M[5] = cos_a + rny * rny * omc
    M[6] = -rnx * sin_a + rny * rnz * omc
    M[7] = ty
    M[8] = -rny * sin_a + rnx * rnz * omc
    M[9] = rnx * sin_a + rny * rnz * omc
    M[10] = cos_a + rnz * rnz * omc
    M[11] = tz
    return M


def cam_center(M):
    i = [M[0], M[4], M[8], None, M[1], M[5], M[9], None, M[2], M[6], M[10], None]
    i[3] = -(M[3] * i[0] + M[7] * i[1] + M[11] * i[2])
    i[7] = -(M[3] * i[4] + M[7] * i[5] + M[11] * i[6])
    i[11] = -(M[3] * i[8] + M[7] * i[9] + M[11] * i[10])
    z = f32(0)
    with np.errstate(all="ignore"):
        return np.array([i[0] * z + i[1] * z + i[2] * z + i[3], i[4] * z + i[5] * z + i[6] * z + i[7], i[8] * z + i[9] * z + i[10] * z + i[11]], f32)


def score(intr4, rt6, p3d, normal, kp):
    """pnpsolver.cpp:75-100 over all matches, float32 in the written order.  Returns (mask, err2, viewcos, margin)."""
    M = se3_set(rt6)
    fx, fy, cx, cy = [f32(v) for v in intr4]
    P, Nn, K = np.asarray(p3d, f32), np.asarray(normal, f32), np.asarray(kp, f32)
    with np.errstate(all="ignore"):
        x = M[0] * P[:, 0] + M[1] * P[:, 1] + M[2] * P[:, 2] + M[3]
        y = M[4] * P[:, 0] + M[5] * P[:, 1] + M[6] * P[:, 2] + M[7]
        z = M[8] * P[:, 0] + M[9] * P[:, 1] + M[10] * P[:, 2] + M[11]
        iz = (1.0 / z.astype(f64)).astype(f32)
        u = ((fx * x) * iz) + cx
        v = ((fy * y) * iz) + cy
        dx = (K[:, 0].astype(f64) - u.astype(f64)).astype(f32)
        dy = (K[:, 1].astype(f64) - v.astype(f64)).astype(f32)
        err2 = dx * dx + dy * dy
        c = cam_center(M)
        w = c[None, :] - P
        s = 1.0 / np.sqrt(w[:, 0].astype(f64) ** 2 + w[:, 1].astype(f64) ** 2 + w[:, 2].astype(f64) ** 2)
        w = (w.astype(f64) * s[:, None]).astype(f32)
        vc = w[:, 0] * Nn[:, 0] + w[:, 1] * Nn[:, 1] + w[:, 2] * Nn[:, 2]
        mask = (err2 < MAX_ERR) & ~(vc < f32(0.5))
        m_err = np.abs(err2.astype(f64) - f64(MAX_ERR)) / f64(MAX_ERR)
        m_vc = np.abs(vc.astype(f64) - 0.5)
        margin = np.where(err2 < MAX_ERR, np.minimum(m_err, m_vc), m_err)
        margin = np.where(np.isfinite(margin), margin, np.inf)
    return mask, err2, vc, margin


def hypothesis(pr, it, intr4=None, jitter=None):
    intr4 = pr["intr"] if intr4 is None else intr4
    idx = np.asarray(pr["samples"][it], np.int64)
    P, px = pr["p3d"][idx].astype(f64), pr["kp"][idx].astype(f64)
    if jitter is not None:
        px = px * (1 + jitter)
    sols, chosen, err = p3p(intr4, P, px)
    return P, px, sols, chosen, err


def ill_conditioned(pr, it, base=None):
    """The project's jitter screening: eight 1e-12 relative jitters of the four pixels change the number of solutions or the chosen
    index, or move the chosen solution by more than 1e-9."""
    _, _, sols, chosen, _ = hypothesis(pr, it) if base is None else base
    rng = np.random.default_rng(12345 + it)
    for _ in range(8):
        _, _, s2, c2, _ = hypothesis(pr, it, jitter=rng.uniform(-JITTER, JITTER, (4, 2)))
        if len(s2) != len(sols) or c2 != chosen:
            return True
        if chosen >= 0:
            scale = 1 + np.abs(sols[chosen]["t"]).max()
            if max(np.abs(s2[c2]["R"] - sols[chosen]["R"]).max(), np.abs(s2[c2]["t"] - sols[chosen]["t"]).max() / scale) > JITTER_MOVE:
                return True
    return False


def run(pr, screen=True):
    """The whole function for one problem dict (pnp_ransac_synth.scene).  Returns dict(hyp = list per iteration of dict(n_solutions,
    solutions, chosen, rvec_tvec (6) f64, rt6 (6) f32, mask, err2, viewcos, margin, count, ill), counts, best_iter, inliers, ok, rt6)."""
    n, iters = pr["n"], pr["iters"]
    hyps, counts = [], np.full(iters, -1, np.int32)
    for it in range(iters):
        base = hypothesis(pr, it)
        P, px, sols, chosen, err = base
        h = dict(n_solutions=len(sols), solutions=sols, chosen=chosen, P=P, px=px, err4=err, ill=ill_conditioned(pr, it, base) if screen else False)
        if chosen >= 0:
            rv = rodrigues_vec(sols[chosen]["R"])
            h["rvec_tvec"] = np.concatenate([rv, sols[chosen]["t"]])
            h["rt6"] = h["rvec_tvec"].astype(f32)
            h["mask"], h["err2"], h["viewcos"], h["margin"] = score(pr["intr"], h["rt6"], pr["p3d"], pr["normal"], pr["kp"])
            h["count"] = int(h["mask"].sum())
            counts[it] = h["count"]
        else:
            h["count"] = -1
            h["margin"] = np.full(n, np.inf)
        hyps.append(h)
    best_iter, best = -1, 0
    for it in range(iters):
        if counts[it] > best:
            best, best_iter = counts[it], it
    inliers = np.nonzero(hyps[best_iter]["mask"])[0].astype(np.int32) if best_iter >= 0 else np.zeros(0, np.int32)
    rt6 = hyps[best_iter]["rt6"] if best_iter >= 0 else np.asarray(pr["rt6_in"], f32)
    return dict(hyp=hyps, counts=counts, best_iter=best_iter, inliers=inliers, n_inliers=len(inliers), ok=int(len(inliers) >= 4), rt6=rt6)
