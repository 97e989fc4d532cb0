"""Deterministic scenes for the new-map-point stage: a new keyframe and K neighbours with known poses, points projected with pixel
noise, octaves assigned, match lists with unique trainIdx per pair.  Everything is a function of the seed."""
from __future__ import annotations

import numpy as np

from newpoints_oracle import DMATCH_DTYPE, _mm

f32 = np.float32
N_LEVELS = 8
SCALE_FACTOR = 1.2
RATIO_FACTOR = float(f32(1.5) * f32(SCALE_FACTOR))   # mapmanager.cpp:10100-10115
SCALE_FACTORS = np.array([f32(SCALE_FACTOR) ** k for k in range(N_LEVELS)], f32)
INTR = np.array([517.3, 516.5, 318.6, 255.3], f32)


def rodrigues(rv):
    rv = np.asarray(rv, np.float64)
    th = np.linalg.norm(rv)
    if th == 0:
        return np.eye(3)
    k = rv / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def pose(rv, center):
    """pose_f2g (global -> camera, float32 4x4) of a camera at `center` with orientation rodrigues(rv)."""
    R = rodrigues(rv)
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = -R @ np.asarray(center, np.float64)
    return M.astype(f32)


def se3_inv(M):
    """Se3Transform::inv (se3transform.h:89-107), float32."""
    M = np.asarray(M, f32).reshape(4, 4)
    o = np.eye(4, dtype=f32)
    o[:3, :3] = M[:3, :3].T
    for r in range(3):
        o[r, 3] = -(M[0, 3] * o[r, 0] + M[1, 3] * o[r, 1] + M[2, 3] * o[r, 2])
    return o


def cam_center(M):
    """Frame::getCameraCenter (frame.h:189-197), float32."""
    p = np.asarray(M, f32).reshape(16)
    return np.array([-(p[3] * p[0] + p[7] * p[4] + p[11] * p[8]), -(p[3] * p[1] + p[7] * p[5] + p[11] * p[9]),
                     -(p[3] * p[2] + p[7] * p[6] + p[11] * p[10])], f32)


def project(pose_f2g, intr4, Xg):
    M = np.asarray(pose_f2g, np.float64)
    Xc = np.asarray(Xg, np.float64) @ M[:3, :3].T + M[:3, 3]
    fx, fy, cx, cy = [float(v) for v in intr4]
    return np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], 1)


def make_new_kf(pose_f2g, pt, octave, intr4=INTR, scale_factors=SCALE_FACTORS):
    return dict(intr4=np.asarray(intr4, f32), scale_factors=np.asarray(scale_factors, f32), pt=np.ascontiguousarray(pt, f32).reshape(-1, 2),
                octave=np.ascontiguousarray(octave, np.int32), pose_f2g=np.asarray(pose_f2g, f32), pose_g2f=se3_inv(pose_f2g),
                cam_center=cam_center(pose_f2g))


def make_pair(new_kf, pose_f2g, pt, octave, matches, intr4=INTR, scale_factors=SCALE_FACTORS):
    """matches: rows (queryIdx = neighbour keypoint, trainIdx = new keyframe's keypoint, distance)."""
    m = np.zeros(len(matches), DMATCH_DTYPE)
    for k, row in enumerate(matches):
        m[k] = (row[0], row[1], 0, row[2] if len(row) > 2 else 10.0 + k)
    RT = _mm(np.asarray(pose_f2g, f32), se3_inv(new_kf["pose_f2g"]))   # mapmanager.cpp:10045-10062
    return dict(RT=RT, intr4=np.asarray(intr4, f32), scale_factors=np.asarray(scale_factors, f32), cam_center=cam_center(pose_f2g),
                pt=np.ascontiguousarray(pt, f32).reshape(-1, 2), octave=np.ascontiguousarray(octave, np.int32), matches=m,
                pose_f2g=np.asarray(pose_f2g, f32))


def scene(seed, n_matches, nk_new, nk_nb, noise=0.4, bad_share=0.12):
    """len(n_matches) neighbours; pair j has n_matches[j] matches (each <= min(nk_new, nk_nb))."""
    rng = np.random.default_rng(seed)
    npts = min(nk_new, nk_nb)
    assert max(n_matches, default=0) <= npts
    new_pose = pose(rng.normal(0, 0.05, 3), rng.normal(0, 0.1, 3))
    Rn = new_pose[:3, :3].astype(np.float64)
    cn = cam_center(new_pose).astype(np.float64)
    # points in front of the new keyframe, inside its image
    depth = rng.uniform(2.5, 9.0, npts)
    px = np.stack([rng.uniform(20, 620, npts), rng.uniform(20, 460, npts)], 1)
    rays = np.stack([(px[:, 0] - INTR[2]) / INTR[0], (px[:, 1] - INTR[3]) / INTR[1], np.ones(npts)], 1)
    Xg = (rays * depth[:, None]) @ Rn + cn
    oct_new = rng.integers(0, N_LEVELS, npts)

    def frame_arrays(pose_f2g, nk, octs):
        perm = rng.permutation(nk)[:npts]                 # point i is keypoint perm[i]
        pt = np.stack([rng.uniform(0, 640, nk), rng.uniform(0, 480, nk)], 1)
        octave = rng.integers(0, N_LEVELS, nk)
        pt[perm] = project(pose_f2g, INTR, Xg) + rng.normal(0, noise, (npts, 2)) * SCALE_FACTORS[octs][:, None]
        octave[perm] = octs
        return perm, pt, octave

    perm_new, pt_new, octave_new = frame_arrays(new_pose, nk_new, oct_new)
    kf = make_new_kf(new_pose, pt_new, octave_new)
    pairs = []
    for j, nm in enumerate(n_matches):
        ang = rng.uniform(0, 2 * np.pi)
        base = rng.uniform(0.4, 1.2)
        c = cn + Rn.T @ np.array([base * np.cos(ang), base * np.sin(ang), rng.normal(0, 0.15)])
        nb_pose = pose(Rn_to_rv(Rn) + rng.normal(0, 0.04, 3), c)
        octs = np.clip(oct_new + rng.integers(-1, 2, npts), 0, N_LEVELS - 1)
        perm, pt, octave = frame_arrays(nb_pose, nk_nb, octs)
        ids = rng.permutation(npts)[:nm]
        q = perm[ids].copy()
        bad = rng.random(nm) < bad_share                  # wrong partners: every refusal branch gets visitors
        q[bad] = rng.integers(0, nk_nb, int(bad.sum()))
        rows = [(int(q[k]), int(perm_new[ids[k]]), float(f32(rng.uniform(5, 80)))) for k in range(nm)]
        pairs.append(make_pair(kf, nb_pose, pt, octave, rows))
    return kf, pairs


def Rn_to_rv(R):
    """rotation vector of a rotation matrix (small angles only: the scenes never turn far)"""
    th = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
    if th < 1e-12:
        return np.zeros(3)
    return th / (2 * np.sin(th)) * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])


# the shapes of tests/test_newpoints.py: name -> (seed, matches per pair, keypoints of the new keyframe, keypoints per neighbour)
CASES = {
    "one_match": (11, [1], 37, 41),
    "m63": (12, [63], 130, 131),
    "m64": (13, [64], 130, 131),
    "m65": (14, [65], 130, 131),
    "empty_pair": (15, [0, 70, 5], 100, 77),
    "wide": (16, [300] * 20, 2000, 2000),
    "one_keypoint": (17, [1, 1], 1, 9),
}


def case(name):
    seed, nm, nk_new, nk_nb = CASES[name]
    return scene(seed, nm, nk_new, nk_nb)
