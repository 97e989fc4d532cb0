"""Deterministic bundle-adjustment problems with stereo / RGB-D observations (the inputs of tests/golden/ba_stereo_golden.npz).

The geometry is synth.ba_problem's (keyframes on a line, KITTI intrinsics, points in front, octave-weighted observations); on top of it
every observation carries a depth as Frame::getDepth would return it: the true camera z with ~0.4 % noise for a share of the
observations, a grossly wrong one (1.6-3 x) for a few of those, 0 (= monocular edge) for the rest; frame_bl = 0.54 m.  Landmarks with
a single observation are kept when that observation has depth (globaloptimizer_g2o.cpp:142) — synth.ba_problem drops them."""
import numpy as np

import synth

INPUT_KEYS = ("poses", "fixed", "intr", "points", "obs_pt", "obs_kf", "obs_uv", "obs_w", "obs_depth", "frame_bl")
BL = 0.54


def stereo_ba_problem(K=8, P=600, seed=0, nfixed=2, stereo_frac=0.6, gross_frac=0.03, single_frac=0.0, depth_noise=0.004, outlier_frac=0.02,
                      pose_noise=0.01, point_noise=0.05, pix_noise=0.5, behind=0, w=1241, h=376):
    """single_frac: share of the landmarks that keep ONE observation, with depth.  behind: so many landmarks start mirrored through the
    centre of one of their cameras (camera-frame z < 0 there)."""
    rng = np.random.default_rng(seed)
    fx = fy = 718.856
    cx, cy = 607.19, 185.22
    Tgt = []
    for k in range(K):
        T = np.eye(4)
        T[:3, 3] = -np.array([0.3 * k, 0.02 * np.sin(k), 0.0])
        Tgt.append(synth._se3_exp(np.r_[0.0, 0.02 * np.sin(0.7 * k), 0.0, 0, 0, 0]) @ T)
    z = rng.uniform(4, 40, P)
    X = np.stack([(rng.uniform(0, w, P) - cx) / fx * z + 0.3 * K / 2, (rng.uniform(0, h, P) - cy) / fy * z, z], 1)
    single = rng.random(P) < single_frac
    obs = []   # (point, frame, u, v, information, depth)
    for p in range(P):
        mine = []
        for k in range(K):
            pc = Tgt[k][:3, :3] @ X[p] + Tgt[k][:3, 3]
            if pc[2] <= 0.5:
                continue
            u, v = fx * pc[0] / pc[2] + cx, fy * pc[1] / pc[2] + cy
            if 0 <= u < w and 0 <= v < h and rng.random() < 0.9:
                octave = int(rng.integers(0, 8))
                noise = rng.normal(0, pix_noise, 2)
                if rng.random() < outlier_frac:
                    noise += rng.normal(0, 25, 2)
                depth = 0.0
                if rng.random() < stereo_frac:
                    depth = pc[2] * (1 + rng.normal(0, depth_noise))
                    if rng.random() < gross_frac:
                        depth *= rng.uniform(1.6, 3.0)
                inv_sigma = float(np.float32(1.0 / float(synth._scale_f32(octave))))   # (double)(float)(1. / f), the reference's _InvScaleFactors
                mine.append([p, k, u + noise[0], v + noise[1], inv_sigma, depth, pc[2]])
        if single[p] and mine:
            keep = mine[int(rng.integers(0, len(mine)))]
            if keep[5] <= 0:
                keep[5] = keep[6] * (1 + rng.normal(0, depth_noise))
            mine = [keep]
        if len(mine) >= 2 or (len(mine) == 1 and mine[0][5] > 0):   # :142: one observer is enough when it is a stereo one
            obs += mine
    poses = []
    fixed = np.zeros(K, np.uint8)
    fixed[:nfixed] = 1
    for k in range(K):
        T = Tgt[k] if fixed[k] else synth._se3_exp(rng.normal(0, pose_noise, 6)) @ Tgt[k]
        poses.append(T.astype(np.float32))
    obs = np.array(obs, np.float64).reshape(-1, 7)
    obs_pt = obs[:, 0].astype(np.int32)
    keep_pt = np.bincount(obs_pt, minlength=P) > 0
    remap = -np.ones(P, np.int32)
    remap[keep_pt] = np.arange(keep_pt.sum(), dtype=np.int32)
    Xn = X + rng.normal(0, point_noise, X.shape)
    obs_kf = obs[:, 1].astype(np.int32)
    for p in rng.permutation(np.flatnonzero(keep_pt))[:behind]:
        k = obs_kf[np.flatnonzero(obs_pt == p)[0]]
        C = -Tgt[k][:3, :3].T @ Tgt[k][:3, 3]
        Xn[p] = C - 0.5 * (Xn[p] - C)
    return dict(
        K=K, P=int(keep_pt.sum()), E=len(obs),
        poses=np.ascontiguousarray(np.stack(poses).reshape(K, 16)), fixed=fixed,
        intr=np.tile(np.array([fx, fy, cx, cy], np.float32), (K, 1)),
        points=np.ascontiguousarray(Xn[keep_pt].astype(np.float32)),
        obs_pt=np.ascontiguousarray(remap[obs_pt]), obs_kf=np.ascontiguousarray(obs_kf),
        obs_uv=np.ascontiguousarray(obs[:, 2:4].astype(np.float32)), obs_w=np.ascontiguousarray(obs[:, 4]),
        obs_depth=np.ascontiguousarray(obs[:, 5].astype(np.float32)), frame_bl=np.full(K, BL, np.float32),
    )


# hard_*: windows that Levenberg-Marquardt does not sail through (rejected trials, lambda factors other than 1/3, passes that end early)
# but that keep a pass 2 worth running — synth.ba_hard_problem's noise levels leave nearly every three-row edge an outlier, so these
# have parameters of their own; the seeds were searched with the real g2o (tests/golden/make_ba_stereo_golden.py --search-hard).
HARD = dict(nfixed=1, pose_noise=0.08, point_noise=0.3, outlier_frac=0.1, pix_noise=1.5, gross_frac=0.08)

CASES = {
    "mix8x600": dict(K=8, P=600, seed=77),
    "rgbd8x600": dict(K=8, P=600, seed=78, stereo_frac=1.0, single_frac=0.2),
    "mono8x600": dict(K=8, P=600, seed=79, stereo_frac=0.0),
    "single_obs": dict(K=8, P=600, seed=80, single_frac=0.34),
    "win20x1500": dict(K=20, P=1500, seed=81),
    "wide70x400": dict(K=70, P=400, seed=82),
    "badz": dict(K=8, P=600, seed=83, behind=6),
    "hard_2": dict(K=10, P=109, seed=2, **HARD),
    "hard_65": dict(K=6, P=69, seed=65, **HARD),
    "hard_169": dict(K=10, P=150, seed=169, **HARD),   # (seed 130 passed the kp_ur probe but not the constants probe: chi2 move 1.15e-6 (1 + max))
}
