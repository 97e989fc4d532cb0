"""numpy restatement of MapInitializer's two-view initialise (src/utils/mapinitializer.cpp:152-201 and what it calls), written from the
reference's text: float32 in the written order (element-wise numpy float32 operations are the scalar IEEE operations; sequential sums
are np.cumsum, which accumulates in order), products through cv::Mat's `*` accumulated in float64 and rounded once, LAPACK SVDs in
float64 under the SIGN RULE of csrc/mapinit_math.hpp, libc's rand through ctypes.

Besides the result it returns what the tests need to tell a disagreement from a tie: per hypothesis the condition sigma_1 / sigma_8 of
its 8-point system, and per (hypothesis, match) / (candidate, match) whether a compared value lies within BAND of its threshold."""
import ctypes
import ctypes.util

import numpy as np

F = np.float32
D = np.float64
BAND = 1e-4
NONE, HOMOGRAPHY, FUNDAMENTAL = 0, 1, 2
NOT_INLIER, REJECTED, COUNTED_LOW, COUNTED_GOOD, NON_FINITE = 0, 1, 2, 3, 4


def draw_samples(n, iterations):
    """:167-182 with libc's rand()"""
    libc = ctypes.CDLL(ctypes.util.find_library("c"))
    libc.srand(0)
    out = np.zeros((iterations, 8), np.int32)
    for it in range(iterations):
        avail = list(range(n))
        for j in range(8):
            r = libc.rand() % len(avail)
            out[it, j] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


def seq_sum(v):
    v = np.asarray(v, F)
    return F(np.cumsum(v, dtype=F)[-1]) if len(v) else F(0)


def normalise(kp):
    """:633-671 -> (mean x, mean y, sX, sY, T)"""
    kp = np.asarray(kp, F)
    n = F(len(kp))
    mx, my = seq_sum(kp[:, 0]) / n, seq_sum(kp[:, 1]) / n
    dx, dy = seq_sum(np.abs(kp[:, 0] - mx)) / n, seq_sum(np.abs(kp[:, 1] - my)) / n
    sx, sy = F(1.0 / D(dx)), F(1.0 / D(dy))
    T = np.array([[sx, 0, -mx * sx], [0, sy, -my * sy], [0, 0, 1]], F)
    return mx, my, sx, sy, T


def mul(A, B):
    """cv::Mat * cv::Mat on CV_32F: each element accumulated in float64 in the order k = 0, 1, 2, rounded once"""
    A, B = np.asarray(A, D), np.asarray(B, D)
    acc = A[:, 0:1] * B[0:1, :]
    for k in range(1, A.shape[1]):
        acc = acc + A[:, k:k + 1] * B[k:k + 1, :]
    return acc.astype(F)


def apply_sign_rule(U, Vt, k):
    i = int(np.argmax(np.abs(Vt[k])))
    if Vt[k, i] < 0:
        Vt[k] = -Vt[k]
        if U is not None and k < U.shape[1]:
            U[:, k] = -U[:, k]


def null_vector(A):
    """the right singular vector of the smallest singular value of the float32 system A (16x9 or 8x9) in float64, and sigma_1 / sigma_8"""
    _, w, Vt = np.linalg.svd(np.asarray(A, F).astype(D), full_matrices=True)
    Vt = Vt.copy()
    apply_sign_rule(None, Vt, 8)
    return Vt[8], (w[0] / w[7] if w[7] > 0 else np.inf)


def svd3(A):
    """A = U diag(w) Vt of a float32 3x3 in float64 under the sign rule (u3 = (u1 x u2) sign(det V) where w3 <= 1e-10 w1)"""
    U, w, Vt = np.linalg.svd(np.asarray(A, F).astype(D))
    U, Vt = U.copy(), Vt.copy()
    for k in range(3):
        apply_sign_rule(U, Vt, k)
    if not w[2] > 1e-10 * w[0]:
        U[:, 2] = np.cross(U[:, 0], U[:, 1]) * (1.0 if np.linalg.det(Vt) >= 0 else -1.0)
    return U, w, Vt


def svd3f(A):
    U, w, Vt = svd3(A)
    return U.astype(F), w.astype(F), Vt.astype(F)


def inv3(M):
    """cv::Mat::inv on a 3x3 CV_32F: adjugate over the determinant in float64, rounded once; zeros where singular"""
    m = np.asarray(M, F).astype(D)
    a, b, c, d, e, f, g, h, i = m.reshape(9)
    det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
    if det == 0:
        return np.zeros((3, 3), F)
    det = 1.0 / det
    return np.array([[(e * i - f * h) * det, (c * h - b * i) * det, (b * f - c * e) * det],
                     [(f * g - d * i) * det, (a * i - c * g) * det, (c * d - a * f) * det],
                     [(d * h - e * g) * det, (b * g - a * h) * det, (a * e - b * d) * det]]).astype(F)


def det3f(m):
    m = np.asarray(m, F)
    return F(m[0, 0] * (m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) - m[0, 1] * (m[1, 0] * m[2, 2] - m[1, 2] * m[2, 0])
             + m[0, 2] * (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]))


def system_h(p1, p2):
    A = np.zeros((16, 9), F)
    for k in range(8):
        u1, v1, u2, v2 = p1[k, 0], p1[k, 1], p2[k, 0], p2[k, 1]
        A[2 * k] = [0, 0, 0, -u1, -v1, -1, v2 * u1, v2 * v1, v2]
        A[2 * k + 1] = [u1, v1, 1, 0, 0, 0, -u2 * u1, -u2 * v1, -u2]
    return A


def system_f(p1, p2):
    A = np.zeros((8, 9), F)
    for k in range(8):
        u1, v1, u2, v2 = p1[k, 0], p1[k, 1], p2[k, 0], p2[k, 1]
        A[k] = [u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1]
    return A


def rank2(Fpre):
    u, w, vt = svd3f(Fpre)
    w = w.copy()
    w[2] = 0
    return mul(mul(u, np.diag(w)), vt)


def score_terms_h(H21, H12, inv_s2, x1, y1, x2, y2):
    th = F(5.991)
    w = (1.0 / (H12[2, 0] * x2 + H12[2, 1] * y2 + H12[2, 2]).astype(D)).astype(F)
    u = (H12[0, 0] * x2 + H12[0, 1] * y2 + H12[0, 2]) * w
    v = (H12[1, 0] * x2 + H12[1, 1] * y2 + H12[1, 2]) * w
    chi1 = ((x1 - u) * (x1 - u) + (y1 - v) * (y1 - v)) * inv_s2
    w = (1.0 / (H21[2, 0] * x1 + H21[2, 1] * y1 + H21[2, 2]).astype(D)).astype(F)
    u = (H21[0, 0] * x1 + H21[0, 1] * y1 + H21[0, 2]) * w
    v = (H21[1, 0] * x1 + H21[1, 1] * y1 + H21[1, 2]) * w
    chi2 = ((x2 - u) * (x2 - u) + (y2 - v) * (y2 - v)) * inv_s2
    return chi1, chi2, th, th


def score_terms_f(Fm, inv_s2, x1, y1, x2, y2):
    a2 = Fm[0, 0] * x1 + Fm[0, 1] * y1 + Fm[0, 2]
    b2 = Fm[1, 0] * x1 + Fm[1, 1] * y1 + Fm[1, 2]
    c2 = Fm[2, 0] * x1 + Fm[2, 1] * y1 + Fm[2, 2]
    num2 = a2 * x2 + b2 * y2 + c2
    chi1 = (num2 * num2 / (a2 * a2 + b2 * b2)) * inv_s2
    a1 = Fm[0, 0] * x2 + Fm[1, 0] * y2 + Fm[2, 0]
    b1 = Fm[0, 1] * x2 + Fm[1, 1] * y2 + Fm[2, 1]
    c1 = Fm[0, 2] * x2 + Fm[1, 2] * y2 + Fm[2, 2]
    num1 = a1 * x1 + b1 * y1 + c1
    chi2 = (num1 * num1 / (a1 * a1 + b1 * b1)) * inv_s2
    return chi1, chi2, F(3.841), F(5.991)


def score(chi1, chi2, th, th_score):
    with np.errstate(invalid="ignore"):
        r1, r2 = chi1 > th, chi2 > th
    t = np.zeros(2 * len(chi1), F)
    t[0::2] = np.where(r1, F(0), th_score - chi1)
    t[1::2] = np.where(r2, F(0), th_score - chi2)
    band = (np.abs(chi1.astype(D) - D(th)) <= BAND * D(th)) | (np.abs(chi2.astype(D) - D(th)) <= BAND * D(th))
    return seq_sum(t), ~(r1 | r2), band


def hypotheses(kp1, kp2, matches, samples, sigma):
    """Every hypothesis of both models: list index 0 = H, 1 = F; each a list over the iterations of dict(M float64 de-normalised in float64,
    Mf float32 as the reference de-normalises it, score, mask, band, cond)."""
    kp1, kp2 = np.asarray(kp1, F), np.asarray(kp2, F)
    mx1, my1, sx1, sy1, T1 = normalise(kp1)
    mx2, my2, sx2, sy2, T2 = normalise(kp2)
    T2inv, T2t = inv3(T2), T2.T.copy()
    T2inv_d = np.array([[1.0 / D(sx2), 0, -D(T2[0, 2]) / D(sx2)], [0, 1.0 / D(sy2), -D(T2[1, 2]) / D(sy2)], [0, 0, 1]])
    x1, y1 = kp1[matches[:, 0], 0], kp1[matches[:, 0], 1]
    x2, y2 = kp2[matches[:, 1], 0], kp2[matches[:, 1], 1]
    n1 = np.stack([(x1 - mx1) * sx1, (y1 - my1) * sy1], 1)
    n2 = np.stack([(x2 - mx2) * sx2, (y2 - my2) * sy2], 1)
    inv_s2 = F(1.0 / D(F(sigma) * F(sigma)))
    out = [[], []]
    for s in samples:
        x, cond = null_vector(system_h(n1[s], n2[s]))
        Hn = x.reshape(3, 3).astype(F)
        H21 = mul(mul(T2inv, Hn), T1)
        H12 = inv3(H21)
        with np.errstate(all="ignore"):
            sc, mask, band = score(*score_terms_h(H21, H12, inv_s2, x1, y1, x2, y2))
        out[0].append(dict(M=T2inv_d @ x.reshape(3, 3) @ T1.astype(D), Mf=H21, score=sc, mask=mask, band=band, cond=cond))
        x, cond = null_vector(system_f(n1[s], n2[s]))
        Fpre = x.reshape(3, 3).astype(F)
        F21 = mul(mul(T2t, rank2(Fpre)), T1)
        U, w, Vt = svd3(Fpre)
        Fd = (U[:, :2] * w[:2]) @ Vt[:2]
        with np.errstate(all="ignore"):
            sc, mask, band = score(*score_terms_f(F21, inv_s2, x1, y1, x2, y2))
        out[1].append(dict(M=T2t.astype(D) @ Fd @ T1.astype(D), Mf=F21, score=sc, mask=mask, band=band, cond=cond))
    return out


def first_best(hyps):
    best, at = F(0), -1
    for i, h in enumerate(hyps):
        if h["score"] > best:
            best, at = h["score"], i
    return at, best


def unit3(v):
    v = np.asarray(v, F)
    s = F(1.0 / np.sqrt(D(v[0]) * D(v[0]) + D(v[1]) * D(v[1]) + D(v[2]) * D(v[2])))
    return v * s


def k_of(intr4):
    fx, fy, cx, cy = (F(v) for v in intr4)
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], F)


def decompose_f(F21, intr4):
    K = k_of(intr4)
    E = mul(mul(K.T.copy(), F21), K)
    u, w, vt = svd3f(E)
    t = unit3(u[:, 2])
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], F)
    R1 = mul(mul(u, W), vt)
    if det3f(R1) < 0:
        R1 = -R1
    R2 = mul(mul(u, W.T.copy()), vt)
    if det3f(R2) < 0:
        R2 = -R2
    return [(R1, t), (R2, t), (R1, -t), (R2, -t)]


def decompose_h(H21, intr4):
    K = k_of(intr4)
    A = mul(mul(inv3(K), H21), K)
    U, w, Vt = svd3f(A)
    s = F(D(det3f(U)) * D(det3f(Vt)))
    d1, d2, d3 = w
    if D(d1 / d2) < 1.00001 or D(d2 / d3) < 1.00001:
        return [], w
    aux1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
    aux3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
    x1 = [aux1, aux1, -aux1, -aux1]
    x3 = [aux3, -aux3, aux3, -aux3]
    out = []

    def cand(Rp, tp):
        m = (D(s) * (U.astype(D)[:, 0:1] * Rp.astype(D)[0:1] + U.astype(D)[:, 1:2] * Rp.astype(D)[1:2] + U.astype(D)[:, 2:3] * Rp.astype(D)[2:3])).astype(F)
        R = mul(m, Vt)
        t = mul(U, tp.reshape(3, 1)).reshape(3)
        return R, unit3(t)

    aux_st = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2)
    ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
    st = [aux_st, -aux_st, -aux_st, aux_st]
    for i in range(4):
        Rp = np.array([[ct, 0, -st[i]], [0, 1, 0], [st[i], 0, ct]], F)
        tp = np.array([x1[i], 0, -x3[i]], F) * (d1 - d3)
        out.append(cand(Rp, tp))
    aux_sp = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2)
    cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
    sp = [aux_sp, -aux_sp, -aux_sp, aux_sp]
    for i in range(4):
        Rp = np.array([[cp, 0, sp[i]], [0, -1, 0], [sp[i], 0, -cp]], F)
        tp = np.array([x1[i], 0, x3[i]], F) * (d1 + d3)
        out.append(cand(Rp, tp))
    return out, w


def check_rt(R, t, intr4, x1, y1, x2, y2, inl, th2):
    """:672-734 over all matches at once -> dict(state, cos, pts, n_good, parallax, band)"""
    fx, fy, cx, cy = (F(v) for v in intr4)
    K = k_of(intr4)
    n = len(x1)
    P2 = mul(K, np.concatenate([R, t.reshape(3, 1)], 1))
    O2 = (-1.0 * (R.astype(D).T[:, 0] * D(t[0]) + R.astype(D).T[:, 1] * D(t[1]) + R.astype(D).T[:, 2] * D(t[2]))).astype(F)
    P1 = np.concatenate([K, np.zeros((3, 1), F)], 1)
    A = np.zeros((n, 4, 4), F)
    with np.errstate(all="ignore"):
        A[:, 0] = x1[:, None] * P1[2][None] - P1[0][None]
        A[:, 1] = y1[:, None] * P1[2][None] - P1[1][None]
        A[:, 2] = x2[:, None] * P2[2][None] - P2[0][None]
        A[:, 3] = y2[:, None] * P2[2][None] - P2[1][None]
    state = np.zeros(n, np.uint8)
    band = np.zeros(n, bool)
    cosv, pts = np.zeros(n, F), np.zeros((n, 3), F)
    idx = np.nonzero(inl)[0]
    fin = np.isfinite(A[idx]).all((1, 2))
    v = np.full((len(idx), 4), np.nan)
    if fin.any():
        v[fin] = np.linalg.svd(A[idx][fin].astype(D))[2][:, 3, :]
    v = v.astype(F)
    with np.errstate(all="ignore"):
        iw = (1.0 / v[:, 3].astype(D)).astype(F)
        X, Y, Z = v[:, 0] * iw, v[:, 1] * iw, v[:, 2] * iw
        finite = np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z)
        n2x, n2y, n2z = X - O2[0], Y - O2[1], Z - O2[2]
        d1 = np.sqrt(X.astype(D) * X + Y.astype(D) * Y + Z.astype(D) * Z).astype(F)
        d2 = np.sqrt(n2x.astype(D) * n2x + n2y.astype(D) * n2y + n2z.astype(D) * n2z).astype(F)
        cosp = ((X.astype(D) * n2x + Y.astype(D) * n2y + Z.astype(D) * n2z) / (d1 * d2).astype(D)).astype(F)
        low = ~(cosp.astype(D) < 0.99998)
        Rd = R.astype(D)
        X2 = (Rd[0, 0] * X + Rd[0, 1] * Y + Rd[0, 2] * Z + D(t[0])).astype(F)
        Y2 = (Rd[1, 0] * X + Rd[1, 1] * Y + Rd[1, 2] * Z + D(t[1])).astype(F)
        Z2 = (Rd[2, 0] * X + Rd[2, 1] * Y + Rd[2, 2] * Z + D(t[2])).astype(F)
        iz1 = (1.0 / Z.astype(D)).astype(F)
        u, w = fx * X * iz1 + cx, fy * Y * iz1 + cy
        e1 = (u - x1[idx]) * (u - x1[idx]) + (w - y1[idx]) * (w - y1[idx])
        iz2 = (1.0 / Z2.astype(D)).astype(F)
        u, w = fx * X2 * iz2 + cx, fy * Y2 * iz2 + cy
        e2 = (u - x2[idx]) * (u - x2[idx]) + (w - y2[idx]) * (w - y2[idx])
        rej = ((Z <= 0) & ~low) | ((Z2 <= 0) & ~low) | (e1 > th2) | (e2 > th2)
        st = np.where(~finite, NON_FINITE, np.where(rej, REJECTED, np.where(low, COUNTED_LOW, COUNTED_GOOD))).astype(np.uint8)
        bd = (np.abs(e1.astype(D) - D(th2)) <= BAND * D(th2)) | (np.abs(e2.astype(D) - D(th2)) <= BAND * D(th2)) \
            | (np.abs(cosp.astype(D) - 0.99998) <= BAND * 0.99998) | (np.abs(Z) <= BAND * d1) | (np.abs(Z2) <= BAND * d2)
    state[idx], band[idx] = st, bd & finite
    cosv[idx] = np.where(finite, cosp, F(0))
    pts[idx] = np.stack([X, Y, Z], 1)
    counted = (state == COUNTED_LOW) | (state == COUNTED_GOOD)
    n_good = int(counted.sum())
    par = F(0)
    if n_good > 0:
        c = np.sort(cosv[counted])
        par = F(np.arccos(D(c[min(50, n_good - 1)])) * 180 / np.pi)
    return dict(state=state, cos=cosv, pts=pts, n_good=n_good, parallax=par, band=band)


def decide(model, cands, N, n_good, par, min_parallax, min_tri):
    if model == FUNDAMENTAL:
        mx = max(n_good[:4])
        n_min = max(int(0.9 * N), min_tri)
        similar = sum(1 for g in n_good[:4] if g > 0.7 * mx)
        winner = list(n_good[:4]).index(mx)
        if mx < n_min or similar > 1:
            return False, winner
        return bool(par[winner] > F(min_parallax)), winner
    if not cands:
        return False, -1
    best, second, winner, bp = 0, 0, -1, F(-1)
    for i in range(8):
        if n_good[i] > best:
            second, best, winner, bp = best, n_good[i], i, par[i]
        elif n_good[i] > second:
            second = n_good[i]
    return bool(second < 0.75 * best and bp >= F(min_parallax) and best > min_tri and best > 0.9 * N), winner


def ratio_bands(model, N, n_good, rh, min_tri):
    """True where a decision ratio (0.40, 0.7, 0.75, 0.9) lies within BAND of its two sides"""
    near = lambda a, b: abs(a - b) <= BAND * max(abs(b), 1e-30)   # noqa: E731
    if near(float(rh), 0.40):
        return True
    g = [int(v) for v in n_good]
    mx = max(g)
    if model == FUNDAMENTAL:
        return any(near(v, 0.7 * mx) for v in g[:4] if mx) or near(mx, 0.9 * N)
    second = sorted(g)[-2]
    return near(second, 0.75 * mx) or near(mx, 0.9 * N)


def empty_result(n_kp1, n):
    return dict(ok=0, model=NONE, winner=-1, best_h=-1, best_f=-1, n_good=np.zeros(8, np.int32), parallax=np.zeros(8, F), n_candidates=0, n_inliers=0,
                matches=np.zeros((0, 2), np.int32), points=np.zeros((0, 3), F), triangulated=np.zeros(n_kp1, bool), state=np.zeros(n, np.uint8))


def initialize(intr4, kp1, kp2, matches, sigma=1.0, iterations=200, min_matches=50, min_parallax=1.0, min_triangulated=50, min_distance=0.1,
               samples=None):
    kp1, kp2, matches = np.asarray(kp1, F).reshape(-1, 2), np.asarray(kp2, F).reshape(-1, 2), np.asarray(matches, np.int32).reshape(-1, 2)
    n = len(matches)
    res = empty_result(len(kp1), n)
    if n < min_matches:
        return res
    if samples is None:
        samples = draw_samples(n, iterations)
    hyps = hypotheses(kp1, kp2, matches, samples, sigma)
    bh, sh = first_best(hyps[0])
    bf, sf = first_best(hyps[1])
    with np.errstate(all="ignore"):
        rh = F(sh / (sh + sf))
    model = HOMOGRAPHY if D(rh) > 0.40 else FUNDAMENTAL
    res.update(hyps=hyps, samples=samples, best_h=bh, best_f=bf, score_h=sh, score_f=sf, rh=rh, model=model)
    at = bh if model == HOMOGRAPHY else bf
    if at < 0:
        return res
    win = hyps[0 if model == HOMOGRAPHY else 1][at]
    return reconstruct(res, intr4, kp1, kp2, matches, model, win["Mf"], win["mask"], rh, sigma, min_parallax, min_triangulated, min_distance)


def reconstruct(res, intr4, kp1, kp2, matches, model, Mf, mask, rh, sigma=1.0, min_parallax=1.0, min_triangulated=50, min_distance=0.1):
    """ReconstructH / ReconstructF on the float model Mf with inlier mask `mask`, and the entry's scatter: fills res"""
    n = len(matches)
    cands = decompose_h(Mf, intr4)[0] if model == HOMOGRAPHY else decompose_f(Mf, intr4)
    x1, y1 = kp1[matches[:, 0], 0], kp1[matches[:, 0], 1]
    x2, y2 = kp2[matches[:, 1], 0], kp2[matches[:, 1], 1]
    sigma2 = F(sigma) * F(sigma)
    th2 = F(4.0 * D(sigma2))
    N = int(np.asarray(mask, bool).sum())
    checks = [check_rt(R, t, intr4, x1, y1, x2, y2, np.asarray(mask, bool), th2) for R, t in cands]
    n_good, par = np.zeros(8, np.int32), np.zeros(8, F)
    for c, ch in enumerate(checks):
        n_good[c], par[c] = ch["n_good"], ch["parallax"]
    ok, winner = decide(model, cands, N, n_good, par, min_parallax, min_triangulated)
    res.update(ok=int(ok), winner=winner, n_good=n_good, parallax=par, n_candidates=len(cands), n_inliers=N if cands else 0, checks=checks, cands=cands,
               ratio_band=bool(cands) and ratio_bands(model, N, n_good, rh, min_triangulated))
    if winner >= 0:
        res["state"] = checks[winner]["state"]
    if not ok:
        return res
    R, t = cands[winner]
    ch = checks[winner]
    tri, p3d = np.zeros(len(kp1), bool), np.zeros((len(kp1), 3), F)
    for j in range(n):
        s, tr = ch["state"][j], matches[j, 0]
        if s == NON_FINITE:
            tri[tr] = False
        if s in (COUNTED_LOW, COUNTED_GOOD):
            p3d[tr] = ch["pts"][j]
        if s == COUNTED_GOOD:
            tri[tr] = True
    keep = tri[matches[:, 0]]
    pose = np.eye(4, dtype=F)
    pose[:3, :3], pose[:3, 3] = R, t * F(min_distance)
    res.update(R=R, t=t, pose=pose, matches=matches[keep].copy(), points=p3d[matches[keep, 0]].copy(), triangulated=tri, p3d=p3d)
    return res
