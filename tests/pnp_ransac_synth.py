"""Deterministic scenes for the relocalisation RANSAC: a planted pose, points at depth 2-10 spread over a 1241x376 image with the
bench's intrinsics, normals towards a plausible mean viewing direction, a chosen share of gross outliers and sub-pixel noise on the
rest.  Everything is a function of the seed."""
from __future__ import annotations

import numpy as np

f32 = np.float32
W, H = 1241, 376
INTR = np.array([718.856, 718.856, 607.19, 185.22], f32)
PIX_NOISE = 0.3


def rodrigues(rv):
    rv = np.asarray(rv, np.float64)
    th = np.linalg.norm(rv)
    if th == 0:
        return np.eye(3)
    k = rv / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def project(R, t, intr4, X):
    Xc = np.asarray(X, np.float64) @ R.T + t
    fx, fy, cx, cy = [float(v) for v in intr4]
    return np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], 1)


def draw_samples(rng, n, iters):
    """iters x 4 distinct indices, by the carried Fisher-Yates shuffle of the reference with the generator given (NOT libc rand())."""
    idx = np.arange(n)
    out = np.zeros((iters, 4), np.int32)
    for it in range(iters):
        for i in range(1, n):
            j = int(rng.integers(0, i + 1))
            idx[i], idx[j] = idx[j], idx[i]
        out[it] = idx[:4]
    return out


def scene(seed, n, iters, outliers=0.3, intr=INTR):
    """dict(n, p3d, normal, kp, iters, samples, rt6_in, planted_rvec, planted_t, planted_inlier (n) bool)."""
    rng = np.random.default_rng(seed)
    rv = rng.normal(0, 0.25, 3)
    R = rodrigues(rv)
    t = rng.normal(0, 0.5, 3)
    fx, fy, cx, cy = [float(v) for v in intr]
    px = np.stack([rng.uniform(20, W - 20, n), rng.uniform(20, H - 20, n)], 1)
    depth = rng.uniform(2, 10, n)
    Xc = np.stack([(px[:, 0] - cx) / fx * depth, (px[:, 1] - cy) / fy * depth, depth], 1)
    X = ((Xc - t) @ R).astype(f32)                      # world = R' (Xc - t)
    centre = -R.T @ t
    # the mean viewing direction of a point seen from a few keyframes near the planted camera
    nrm = centre + rng.normal(0, 0.4, (n, 3)) - X.astype(np.float64)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    kp = project(R, t, intr, X.astype(np.float64)) + rng.normal(0, PIX_NOISE, (n, 2))
    bad = np.zeros(n, bool)
    n_out = int(round(outliers * n))
    if n_out:
        which = rng.choice(n, n_out, replace=False)
        bad[which] = True
        # a gross outlier: somewhere else in the image, at least 30 px away
        for i in which:
            while True:
                q = np.array([rng.uniform(0, W), rng.uniform(0, H)])
                if np.linalg.norm(q - kp[i]) > 30:
                    break
            kp[i] = q
    return dict(n=n, p3d=np.ascontiguousarray(X), normal=np.ascontiguousarray(nrm.astype(f32)), kp=np.ascontiguousarray(kp.astype(f32)), iters=iters,
                samples=draw_samples(rng, n, iters), rt6_in=np.array([0.01, -0.02, 0.03, 0.1, 0.2, 0.3], f32), planted_rvec=rv, planted_R=R,
                planted_t=t, planted_inlier=~bad, intr=np.asarray(intr, f32))


# the scenes of the parity tests: (seed, n, iters, outlier share).  n covers the mask word and wave-stride edges, iters the
# four-waves-per-workgroup edge.
SIZES = (4, 5, 63, 64, 65, 129, 257, 1000)
ITERS = (1, 3, 4, 5, 50)
PARITY = {f"n{n}_it{it}": (100 + 7 * k, n, it, 0.0 if n < 16 else 0.3)
          for k, (n, it) in enumerate([(4, 1), (5, 3), (63, 4), (64, 5), (65, 50), (129, 4), (257, 5), (1000, 50), (64, 1), (65, 3)])}
PLANTED = {"out30": (301, 300, 50, 0.3), "out60": (302, 300, 50, 0.6)}


def parity_scene(name):
    return scene(*PARITY[name])


def planted_scene(name):
    return scene(*PLANTED[name])
