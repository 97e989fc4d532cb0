"""Deterministic bundle-adjustment windows in which no two keyframes share a camera (the inputs of tests/golden/ba_het_golden.npz).

stereo_ba_synth.stereo_ba_problem's geometry, noise model, single-observer rule and output keys, but
  - every keyframe has its own intrinsics row (fx != fy, principal point off the nominal one) and its own stereo baseline, all
    rounded to float32 as the ABI takes them; an observation is projected with its own frame's row;
  - the cameras turn about all three axes (up to 0.08 / 0.1 / 0.15 rad), not about y alone;
  - the fixed keyframes are named one by one (fixed_idx) and are never a prefix, so a keyframe's index and its free slot differ;
  - the observation list is shuffled: neither point-major nor ascending in the keyframe.
A kernel that reads row 0 of a per-frame table, swaps fx and fy, or takes a keyframe index for a free slot computes something else
on these windows (tests/golden/make_ba_het_golden.py measures by how much with the real g2o, condition 4)."""
import numpy as np

import synth
from stereo_ba_synth import INPUT_KEYS  # noqa: F401  (same keys, same digest helper)

FX, CX, CY = 718.856, 607.19, 185.22
BL = 0.54


def cameras(K, rng, bl_spread=0.4):
    """(intr [K,4] f32, frame_bl [K] f32): one draw per keyframe, in the order fx, fy, cx, cy, baseline."""
    intr = np.zeros((K, 4), np.float32)
    bl = np.zeros(K, np.float32)
    for k in range(K):
        fx = FX * (1 + 0.12 * rng.uniform(-1, 1))
        fy = fx * (1 + 0.06 * rng.uniform(-1, 1))
        intr[k] = [fx, fy, CX + rng.uniform(-25, 25), CY + rng.uniform(-15, 15)]
        bl[k] = BL * (1 + bl_spread * rng.uniform(-1, 1))
    return intr, bl


def true_poses(K):
    Tgt = []
    for k in range(K):
        T = np.eye(4)
        T[:3, 3] = -np.array([0.3 * k, 0.02 * np.sin(k), 0.0])
        Tgt.append(synth._se3_exp(np.r_[0.08 * np.sin(1.3 * k), 0.1 * np.sin(0.7 * k), 0.15 * np.cos(0.9 * k), 0, 0, 0]) @ T)
    return Tgt


def het_ba_problem(K=8, P=600, seed=0, fixed_idx=(2, 5), stereo_frac=0.6, gross_frac=0.03, single_frac=0.0, depth_noise=0.004, outlier_frac=0.02,
                   pose_noise=0.01, point_noise=0.05, pix_noise=0.5, bl_spread=0.4, w=1241, h=376):
    fixed_idx = tuple(int(k) for k in fixed_idx)
    assert fixed_idx and all(0 <= k < K for k in fixed_idx) and len(set(fixed_idx)) == len(fixed_idx)
    assert sorted(fixed_idx) != list(range(len(fixed_idx))), "the fixed keyframes must not be a prefix"
    rng = np.random.default_rng(seed)
    intr, frame_bl = cameras(K, rng, bl_spread)
    I = intr.astype(np.float64)      # the rounded values are the camera: observations are exact projections with what the solver is given
    Tgt = true_poses(K)
    z = rng.uniform(4, 40, P)
    X = np.stack([(rng.uniform(0, w, P) - CX) / FX * z + 0.3 * K / 2, (rng.uniform(0, h, P) - CY) / FX * z, z], 1)
    single = rng.random(P) < single_frac
    obs = []   # (point, frame, u, v, information, depth, true z)
    for p in range(P):
        mine = []
        for k in range(K):
            pc = Tgt[k][:3, :3] @ X[p] + Tgt[k][:3, 3]
            if pc[2] <= 0.5:
                continue
            u, v = I[k, 0] * pc[0] / pc[2] + I[k, 2], I[k, 1] * pc[1] / pc[2] + I[k, 3]
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
        if len(mine) >= 2 or (len(mine) == 1 and mine[0][5] > 0):   # one observer is enough when it is a stereo one
            obs += mine
    fixed = np.zeros(K, np.uint8)
    fixed[list(fixed_idx)] = 1
    poses = []
    for k in range(K):
        T = Tgt[k] if fixed[k] else synth._se3_exp(rng.normal(0, pose_noise, 6)) @ Tgt[k]
        poses.append(T.astype(np.float32))
    obs = np.array(obs, np.float64).reshape(-1, 7)
    obs = obs[rng.permutation(len(obs))]                              # neither point-major nor ascending in the keyframe
    obs_pt = obs[:, 0].astype(np.int32)
    keep_pt = np.bincount(obs_pt, minlength=P) > 0
    remap = -np.ones(P, np.int32)
    remap[keep_pt] = np.arange(keep_pt.sum(), dtype=np.int32)
    Xn = X + rng.normal(0, point_noise, X.shape)
    return dict(
        K=K, P=int(keep_pt.sum()), E=len(obs),
        poses=np.ascontiguousarray(np.stack(poses).reshape(K, 16)), fixed=fixed, intr=intr,
        points=np.ascontiguousarray(Xn[keep_pt].astype(np.float32)),
        obs_pt=np.ascontiguousarray(remap[obs_pt]), obs_kf=np.ascontiguousarray(obs[:, 1].astype(np.int32)),
        obs_uv=np.ascontiguousarray(obs[:, 2:4].astype(np.float32)), obs_w=np.ascontiguousarray(obs[:, 4]),
        obs_depth=np.ascontiguousarray(obs[:, 5].astype(np.float32)), frame_bl=frame_bl,
    )


def unequal_cameras(pr, rng):
    """A copy of a window of synth.ba_problem / stereo_ba_problem (one camera, fixed prefix) with cameras() drawn per keyframe, every
    observation moved to where its own frame's camera sees the same ray, and as many fixed keyframes at random places
    (scripts/fuzz_parity.py: the randomised sweep's BA windows)."""
    K = pr["K"]
    m = dict(pr)
    intr, bl = cameras(K, rng)
    old, new = pr["intr"].astype(np.float64)[pr["obs_kf"]], intr.astype(np.float64)[pr["obs_kf"]]
    m["obs_uv"] = np.ascontiguousarray(((pr["obs_uv"].astype(np.float64) - old[:, 2:4]) / old[:, 0:2] * new[:, 0:2] + new[:, 2:4]).astype(np.float32))
    m["intr"] = intr
    if "frame_bl" in pr:
        m["frame_bl"] = bl
    m["fixed"] = np.zeros(K, np.uint8)
    m["fixed"][rng.choice(K, int(pr["fixed"].sum()), replace=False)] = 1
    if "poses_gt" in pr:                                               # a fixed keyframe stands where it truly is, as in the generators
        m["poses"] = pr["poses"].copy()
        gt = np.asarray(pr["poses_gt"]).reshape(K, 16).astype(np.float32)
        m["poses"][m["fixed"] != 0] = gt[m["fixed"] != 0]
    return m


# ------------------------------------------------------------------------------------------------ the faults the cases are for
def mutant(pr, which):
    """The window a wrong kernel would in effect solve: 'intr0' (row 0 of the intrinsics for every keyframe), 'fxfy' (fx and fy
    swapped), 'bl0' (the first keyframe's baseline for all), 'prefix' (as many fixed keyframes, but the first ones)."""
    m = dict(pr)
    if which == "intr0":
        m["intr"] = np.ascontiguousarray(np.tile(pr["intr"][:1], (pr["K"], 1)))
    elif which == "fxfy":
        m["intr"] = np.ascontiguousarray(pr["intr"][:, [1, 0, 2, 3]])
    elif which == "bl0":
        m["frame_bl"] = np.full(pr["K"], pr["frame_bl"][0], np.float32)
    elif which == "prefix":
        m["fixed"] = np.zeros(pr["K"], np.uint8)
        m["fixed"][:int(pr["fixed"].sum())] = 1
    else:
        raise KeyError(which)
    return m


MUTANTS = ("intr0", "fxfy", "bl0", "prefix")


# ------------------------------------------------------------------------------------------------ which form a window runs in
def planned_form(nfree, stereo):
    """The optimiser's plan for a window of nfree free keyframes with its defaults (ba.hip: plan_ba)."""
    if nfree > 64:
        return "wide"
    if stereo or nfree > 16:
        return "chain"
    return "persist8" if nfree <= 8 else "persist16"


def dense_wide_nown(nfree):
    """Tiles per wave of ba_schur_dense_wide_kernel (instantiated for 12, 16 and 20) for 33-64 free keyframes: the reduced system's
    upper triangle of 16 x 16 tiles, cut over workgroups of at most 80 tiles, four waves each."""
    assert 32 < nfree <= 64
    ntt = -(-6 * nfree // 16)
    T = ntt * (ntt + 1) // 2
    SP = -(-T // 80)
    need = -(-(-(-T // SP)) // 4)
    return 12 if need <= 12 else (16 if need <= 16 else 20)


# name: generator arguments.  FORMS: the form each must plan, the Schur kernel of the chain cases, nown of the dense-wide ones.
CASES = {
    "het8": dict(K=8, P=420, seed=301, fixed_idx=(2, 5)),
    "het8_mono": dict(K=8, P=420, seed=302, fixed_idx=(0, 7), stereo_frac=0.0),
    "het14_mono": dict(K=14, P=330, seed=303, fixed_idx=(2, 9), stereo_frac=0.0),
    "het10_one_fixed_last": dict(K=10, P=380, seed=304, fixed_idx=(9,), stereo_frac=0.0),
    "het18": dict(K=18, P=280, seed=325, fixed_idx=(3, 17)),     # (seed 305 failed the constants probe: chi2 move 9.98e-7 (1 + max))
    "het19": dict(K=19, P=280, seed=326, fixed_idx=(0, 9)),      # (seed 306 failed the 1e-9 px probe)
    "het35": dict(K=35, P=200, seed=307, fixed_idx=(4, 20)),
    "het_rgbd35": dict(K=35, P=240, seed=308, fixed_idx=(3, 34), stereo_frac=1.0, single_frac=0.2),
    "het42": dict(K=42, P=180, seed=309, fixed_idx=(1, 30)),
    "het50": dict(K=50, P=160, seed=310, fixed_idx=(7, 49)),
    "het66": dict(K=66, P=130, seed=311, fixed_idx=(10, 65)),
    "het67": dict(K=67, P=130, seed=312, fixed_idx=(0, 40)),
}
FORMS = {   # name: (free keyframes, planned form, Schur kernel of the chain, nown)
    "het8": (6, "chain", "pair", None),
    "het8_mono": (6, "persist8", None, None),
    "het14_mono": (12, "persist16", None, None),
    "het10_one_fixed_last": (9, "persist16", None, None),
    "het18": (16, "chain", "pair", None),
    "het19": (17, "chain", "dense", None),
    "het35": (33, "chain", "dense-wide", 12),
    "het_rgbd35": (33, "chain", "dense-wide", 12),
    "het42": (40, "chain", "dense-wide", 16),
    "het50": (48, "chain", "dense-wide", 16),
    "het66": (64, "chain", "dense-wide", 20),
    "het67": (65, "wide", None, None),
}
MONO_CASES = ("het8_mono", "het14_mono", "het10_one_fixed_last")

# the stereo window of the bench size (scripts/time_ba_stereo.py): only state, iterations and a digest of the flags are recorded
BENCH_CASE = ("mix10x3000", dict(K=10, P=3000, seed=320, fixed_idx=(3, 8)))
