"""Synthetic pose-only problems with squared planar markers (PnPSolver::solvePnp with frame.markers, pnpsolver.cpp:280-347).

Keypoint matches as synth.pnp_problem / stereo_synth.stereo_pnp_problem make them, plus n_markers markers in front of the true camera:
Marker::pose_g2m stored as float (row-major 4x4), Marker::size, and MarkerObservation::und_corners = the projection of the four corners
(order of Marker::get3DPointsLocalRefSystem) with pixel noise, as float."""
import numpy as np

import stereo_synth
import synth

MARKER_KEYS = ("pose_g2m", "size", "und_corners")


def _rot(w):
    T = synth._se3_exp(np.r_[w, 0, 0, 0])
    return T[:3, :3]


def make_markers(rng, Tgt, intr, n_markers, corner_noise=0.5):
    """n_markers markers in front of the camera whose true pose (global -> camera, 4x4) is Tgt: dict(pose_g2m [m,16], size [m],
    und_corners [m,8]), all float32."""
    fx, fy, cx, cy = (float(v) for v in intr)
    g2m = np.zeros((n_markers, 16), np.float32)
    size = np.zeros(n_markers, np.float32)
    corners = np.zeros((n_markers, 8), np.float32)
    for m in range(n_markers):
        z = rng.uniform(2.0, 6.0)
        centre = np.array([(rng.uniform(200, 1000) - cx) / fx * z, (rng.uniform(80, 300) - cy) / fy * z, z])
        c2m = np.eye(4)
        # the marker faces the camera (its z axis towards it: a half turn about x) with a tilt of up to ~0.5 rad
        c2m[:3, :3] = _rot(rng.uniform(-0.5, 0.5, 3)) @ _rot(np.array([np.pi, 0, 0]))
        c2m[:3, 3] = centre
        G = (np.linalg.inv(Tgt) @ c2m).astype(np.float32)
        g2m[m] = G.reshape(16)
        s = np.float32(rng.uniform(0.1, 0.3))
        size[m] = s
        h = float(s) / 2
        P = np.array([[-h, h, 0, 1], [h, h, 0, 1], [h, -h, 0, 1], [-h, -h, 0, 1]])
        Pc = (Tgt @ G.astype(np.float64) @ P.T).T
        uv = np.stack([fx * Pc[:, 0] / Pc[:, 2] + cx, fy * Pc[:, 1] / Pc[:, 2] + cy], 1) + rng.normal(0, corner_noise, (4, 2))
        corners[m] = uv.reshape(8).astype(np.float32)
    return dict(pose_g2m=g2m, size=size, und_corners=corners)


def marker_pnp_problem(n, n_markers, seed=0, stereo=False, corner_noise=0.5, **kw):
    """The keypoint problem (stereo=True: with depths) plus `markers` = make_markers(...).  depth is None for a monocular problem."""
    if stereo:
        pr = stereo_synth.stereo_pnp_problem(n, seed, **kw)
    else:
        pr = synth.pnp_problem(n, seed, **kw)
        pr.update(depth=None, bl=np.float32(0.0))
    pr["markers"] = make_markers(np.random.default_rng(20_000 + seed), pr["pose_gt"], pr["intr"], n_markers, corner_noise)
    return pr


# the fixture's cases (tests/golden/pnp_marker_golden.npz): name -> keyword arguments of marker_pnp_problem.  A seed is replaced when
# tests/golden/make_pnp_marker_golden.py says that the case does not pass its jitter screen.
CASES = {
    "kp300_m2": dict(n=300, n_markers=2, seed=51),
    "kp40_m1": dict(n=40, n_markers=1, seed=42),
    "kp5_m2": dict(n=5, n_markers=2, seed=43, outlier_frac=0.0),              # below the 10-inlier stop, which must not fire
    "out97_m2": dict(n=300, n_markers=2, seed=54, outlier_frac=0.97),         # fewer than 10 good matches, all four rounds run
    "m1_far": dict(n=0, n_markers=1, seed=45, pose_noise=0.08),               # inf weight: one rejected trial, then the kernel is dropped
    "m2_close": dict(n=0, n_markers=2, seed=46, pose_noise=2e-4),             # the kernel survives until the round rule removes it
    "noisy_m2": dict(n=300, n_markers=2, seed=47, corner_noise=30.0),         # the kernel is dropped by the chi2 rule
    "mix500_m3": dict(n=500, n_markers=3, seed=48, stereo=True),
    "kp3001_m3": dict(n=3001, n_markers=3, seed=49),                          # beyond the LDS-resident 3000: the solver's HBM form
    "kp300_m0": dict(n=300, n_markers=0, seed=50),
}

INPUT_KEYS = ("pose", "intr", "p3d", "kp", "invsig", "weight")
