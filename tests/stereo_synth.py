"""Synthetic stereo / RGB-D pose-only problems (PnPSolver::solvePnp with Frame::getDepth > 0 for some matches, pnpsolver.cpp:205-276).

Built on synth.pnp_problem (the monocular problem: map points, keypoints with pixel noise and gross outliers, octave information,
half-weight unstable points); each match then gets a depth: the true camera z with a little noise for a share of the matches, a grossly
wrong depth for a few of those (the right-image residual exceeds Chi3D: they are relabelled as outliers), 0 (monocular) for the rest."""
import numpy as np

import synth

BL = 0.54   # stereo baseline in metres (a KITTI-like rig; fx = 718.856 in synth.pnp_problem)


def stereo_pnp_problem(n, seed=0, stereo_frac=0.6, bad_depth_frac=0.08, depth_noise=0.004, **kw):
    """synth.pnp_problem(n, seed, **kw) plus depth [n] float32 and bl.  stereo_frac of the matches carry a depth; bad_depth_frac of
    those a depth 1.6x-3x off."""
    pr = synth.pnp_problem(n, seed, **kw)
    rng = np.random.default_rng(10_000 + seed)
    Tgt = pr["pose_gt"]
    zc = pr["p3d"].astype(np.float64) @ Tgt[2, :3] + Tgt[2, 3]            # true camera z of each map point
    stereo = rng.random(n) < stereo_frac
    depth = zc * (1.0 + rng.normal(0, depth_noise, n))
    gross = stereo & (rng.random(n) < bad_depth_frac)
    depth[gross] *= rng.uniform(1.6, 3.0, int(gross.sum()))
    depth = np.where(stereo, depth, 0.0).astype(np.float32)
    pr.update(depth=depth, bl=np.float32(BL), stereo=stereo, bad_depth=gross)
    return pr


# the fixture's cases (tests/golden/pnp_stereo_golden.npz): name -> keyword arguments of stereo_pnp_problem
CASES = {
    "mix500": dict(n=500, seed=31),
    "mix1300": dict(n=1300, seed=32),
    "mix3001": dict(n=3001, seed=33),                                  # beyond the LDS-resident 3000: the solver's HBM form
    "stereo800": dict(n=800, seed=34, stereo_frac=1.0),
    "mono600": dict(n=600, seed=35, stereo_frac=0.0),
    "early14": dict(n=14, seed=36, outlier_frac=0.7, pose_noise=0.08),   # fewer than 10 inliers: the rounds stop early
}

INPUT_KEYS = ("pose", "intr", "p3d", "kp", "invsig", "weight", "depth")
