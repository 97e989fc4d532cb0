#!/usr/bin/env python3
"""Writes tests/golden/mapinit_golden.npz: the mathematical contract of the map initialiser's linear algebra at 60 digits (mpmath), on
float32 inputs taken exactly.  What csrc/mapinit_math.hpp computes in float64 / float32 is compared with these in
tests/test_mapinit_host.py.

  null_h / null_f   the null direction (unit norm, largest component positive) of 8-point systems built from NORMALISED float32 point
                    pairs: general and planar samples, three and four collinear points, all eight on one plane (F), with the gap
                    sigma_8 - sigma_9 relative to sigma_1 that conditions it
  rank2             the rank-2 projection U diag(s1, s2, 0) V^T of float32 3x3 matrices
  dec_f             E = K^T F K -> R1, R2 (determinant +1) and the unit t of float32 F; the four candidates are (R1 | R2, +t | -t)
  dec_h             A = K^-1 H K -> singular values, whether d1/d2 < 1.00001 or d2/d3 < 1.00001 (ratios planted near that exit on both
                    sides and for both pairs), and Faugeras' eight (R, t) otherwise
  tri               the triangulated point of one match under P1 = [K | 0], P2 = K [R | t]

    python tests/golden/make_mapinit_golden.py"""
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 60
F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
K = np.array([[500, 0, 320], [0, 500, 240], [0, 0, 1]], F)


def M(a):
    a = np.asarray(a)
    return mp.matrix([[mp.mpf(float(v)) for v in row] for row in a.reshape(a.shape[0], -1)])


def to_np(m):
    return np.array([[float(m[i, j]) for j in range(m.cols)] for i in range(m.rows)])


def unit_positive(v):
    v = np.array([mp.mpf(x) for x in v], dtype=object)
    n = mp.sqrt(sum(x * x for x in v))
    v = v / n
    i = int(np.argmax([abs(x) for x in v]))
    return np.array([float(x if v[i] > 0 else -x) for x in v])


def null_of(A):
    _, S, V = mp.svd_r(M(A), full_matrices=True)
    s = [S[i] for i in range(len(S))] + [mp.mpf(0)] * (9 - len(S))
    return unit_positive([V[8, j] for j in range(9)]), float((s[7] - s[8]) / s[0])


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


def views(rng, kind):
    """eight normalised point pairs (zero mean, unit mean deviation up to sampling) of a two-view scene"""
    xy = rng.uniform(-1.5, 1.5, (8, 2))
    if kind == "collinear3":
        xy[2] = 0.5 * (xy[0] + xy[1])
    if kind == "collinear4":
        xy[2], xy[3] = 0.5 * (xy[0] + xy[1]), 0.25 * xy[0] + 0.75 * xy[1]
    # the plane Z = 5 + 0.3 X - 0.2 Y met by the ray through (xy / 5, 1): Z = 5 / (1 - (0.3 x - 0.2 y) / 5)
    z = 5.0 / (1.0 - (0.3 * xy[:, 0] - 0.2 * xy[:, 1]) / 5.0) if kind in ("planar", "plane8") else rng.uniform(4, 8, 8)
    P = np.concatenate([xy * (z[:, None] / 5.0), z[:, None]], 1)
    a = 0.04
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Q = P @ R.T + np.array([0.5, 0.05, 0.02])
    p1, p2 = P[:, :2] / P[:, 2:3], Q[:, :2] / Q[:, 2:3]
    if kind not in ("plane8",):
        p1, p2 = p1 + rng.normal(0, 2e-4, p1.shape), p2 + rng.normal(0, 2e-4, p2.shape)
    return (4 * p1).astype(F), (4 * (p2 - p2.mean(0))).astype(F)


def svd3(A):
    U, S, V = mp.svd_r(M(A), full_matrices=True)
    return U, [S[i] for i in range(3)], V


def main():
    rng = np.random.default_rng(2026)
    out = {}
    kinds_h = ["general"] * 4 + ["planar"] * 4 + ["collinear3"] * 2
    kinds_f = ["general"] * 4 + ["planar"] * 2 + ["collinear3"] * 2 + ["collinear4"] * 2 + ["plane8"] * 2
    sys_h, nv_h, gap_h = [], [], []
    for kind in kinds_h:
        A = system_h(*views(rng, kind))
        x, g = null_of(A)
        sys_h.append(A); nv_h.append(x); gap_h.append(g)
    sys_f, nv_f, gap_f = [], [], []
    for kind in kinds_f:
        A = system_f(*views(rng, kind))
        x, g = null_of(A)
        sys_f.append(A); nv_f.append(x); gap_f.append(g)
    out.update(null_h_A=np.array(sys_h), null_h_x=np.array(nv_h), null_h_gap=np.array(gap_h), null_h_kind=np.array(kinds_h),
               null_f_A=np.array(sys_f), null_f_x=np.array(nv_f), null_f_gap=np.array(gap_f), null_f_kind=np.array(kinds_f))
    # rank 2
    r_in, r_out = [], []
    for k in range(8):
        A = rng.normal(size=(3, 3)).astype(F)
        U, s, V = svd3(A)
        P = U * mp.diag([s[0], s[1], 0]) * V
        r_in.append(A); r_out.append(to_np(P))
    out.update(rank2_in=np.array(r_in), rank2_out=np.array(r_out))
    # decomposition of F
    Km = M(K)
    f_in, f_R1, f_R2, f_t = [], [], [], []
    for k in range(6):
        a = rng.normal(0, 0.05, 3)
        Rt = to_np(mp.expm(M(np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]]))))
        t = rng.normal(size=3); t /= np.linalg.norm(t)
        tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
        Kinv = np.linalg.inv(K.astype(np.float64))
        F21 = (Kinv.T @ tx @ Rt @ Kinv)
        F21 = (F21 / np.abs(F21).max()).astype(F)
        E = Km.T * M(F21) * Km
        U, s, V = mp.svd_r(E, full_matrices=True)
        W = mp.matrix([[0, -1, 0], [1, 0, 0], [0, 0, 1]])
        R1, R2 = U * W * V, U * W.T * V
        if mp.det(R1) < 0:
            R1 = -R1
        if mp.det(R2) < 0:
            R2 = -R2
        u3 = [U[i, 2] for i in range(3)]
        n = mp.sqrt(sum(x * x for x in u3))
        f_in.append(F21); f_R1.append(to_np(R1)); f_R2.append(to_np(R2)); f_t.append([float(x / n) for x in u3])
    out.update(dec_f_in=np.array(f_in), dec_f_R1=np.array(f_R1), dec_f_R2=np.array(f_R2), dec_f_t=np.array(f_t))
    # decomposition of H: general cases, and singular-value ratios planted at 1.00001 -+ 5e-6 for (d1, d2) and for (d2, d3)
    h_in, h_d, h_exit, h_R, h_t = [], [], [], [], []
    plans = [None] * 4 + [(1.000015, 1.3), (1.000005, 1.3), (1.3, 1.000015), (1.3, 1.000005)]
    for plan in plans:
        if plan is None:
            a = rng.normal(0, 0.05, 3)
            R = to_np(mp.expm(M(np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]]))))
            t, nrm = rng.normal(0, 0.15, 3), rng.normal(size=3) + np.array([0, 0, 3.0])
            A = R + np.outer(t, nrm / np.linalg.norm(nrm))
        else:
            Q1, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            Q2, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            A = Q1 @ np.diag([plan[0] * plan[1], plan[1], 1.0]) @ Q2.T
        H = (K.astype(np.float64) @ A @ np.linalg.inv(K.astype(np.float64)))
        H = (H / np.abs(H).max()).astype(F)
        Am = mp.inverse(Km) * M(H) * Km
        U, s, Vt = mp.svd_r(Am, full_matrices=True)
        d1, d2, d3 = s[0], s[1], s[2]
        ex = bool(d1 / d2 < mp.mpf("1.00001") or d2 / d3 < mp.mpf("1.00001"))
        Rs, ts = np.zeros((8, 3, 3)), np.zeros((8, 3))
        if not ex:
            sg = mp.det(U) * mp.det(Vt)
            aux1, aux3 = mp.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3)), mp.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
            x1, x3 = [aux1, aux1, -aux1, -aux1], [aux3, -aux3, aux3, -aux3]
            ast = mp.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2)
            ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
            st = [ast, -ast, -ast, ast]
            asp = mp.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2)
            cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
            sp = [asp, -asp, -asp, asp]
            for i in range(8):
                j = i % 4
                if i < 4:
                    Rp = mp.matrix([[ct, 0, -st[j]], [0, 1, 0], [st[j], 0, ct]])
                    tp = mp.matrix([x1[j], 0, -x3[j]]) * (d1 - d3)
                else:
                    Rp = mp.matrix([[cp, 0, sp[j]], [0, -1, 0], [sp[j], 0, -cp]])
                    tp = mp.matrix([x1[j], 0, x3[j]]) * (d1 + d3)
                Rm = sg * U * Rp * Vt
                tm = U * tp
                tm = tm / mp.norm(tm)
                Rs[i], ts[i] = to_np(Rm), [float(tm[r]) for r in range(3)]
        h_in.append(H); h_d.append([float(d1), float(d2), float(d3)]); h_exit.append(ex); h_R.append(Rs); h_t.append(ts)
    out.update(dec_h_in=np.array(h_in), dec_h_d=np.array(h_d), dec_h_exit=np.array(h_exit), dec_h_R=np.array(h_R), dec_h_t=np.array(h_t))
    # triangulation
    t_R, t_t, t_xy, t_X = [], [], [], []
    for k in range(8):
        a = 0.03 + 0.01 * k
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]).astype(F)
        t = np.array([0.9, 0.1 * (k % 3), 0.05], F)
        t = (t / F(np.linalg.norm(t))).astype(F)
        X = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(3, 6)])
        q = R.astype(np.float64) @ X + t
        xy = np.array([500 * X[0] / X[2] + 320, 500 * X[1] / X[2] + 240, 500 * q[0] / q[2] + 320, 500 * q[1] / q[2] + 240]) + rng.normal(0, 0.2, 4)
        xy = xy.astype(F)
        P2f = (K.astype(np.float64) @ np.concatenate([R, t.reshape(3, 1)], 1).astype(np.float64)).astype(F)   # the float32 P2 the reference triangulates with
        P1 = M(np.concatenate([K, np.zeros((3, 1), F)], 1))
        P2 = M(P2f)
        A = mp.matrix(4, 4)
        for c in range(4):
            A[0, c] = mp.mpf(float(xy[0])) * P1[2, c] - P1[0, c]
            A[1, c] = mp.mpf(float(xy[1])) * P1[2, c] - P1[1, c]
            A[2, c] = mp.mpf(float(xy[2])) * P2[2, c] - P2[0, c]
            A[3, c] = mp.mpf(float(xy[3])) * P2[2, c] - P2[1, c]
        _, _, V = mp.svd_r(A, full_matrices=True)
        t_R.append(R); t_t.append(t); t_xy.append(xy); t_X.append([float(V[3, c] / V[3, 3]) for c in range(3)])
    out.update(tri_R=np.array(t_R), tri_t=np.array(t_t), tri_xy=np.array(t_xy), tri_X=np.array(t_X))
    np.savez_compressed(os.path.join(HERE, "mapinit_golden.npz"), **out)
    print({k: np.asarray(v).shape for k, v in out.items()})
    print("null_h gaps", np.array(gap_h), "\nnull_f gaps", np.array(gap_f), "\nexits", h_exit)


if __name__ == "__main__":
    main()
