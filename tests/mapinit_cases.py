"""Scenes of the map-initialiser tests: two synthetic views of planted points, with the oracle's result computed once per scene and
shared by tests/test_mapinit_host.py (CPU) and tests/test_mapinit.py (GPU).

Camera: 640 x 480, f = 500.  The second camera is planted at (R, t) with |t| = 0.5 in front of points 4 to 8 units deep, which gives
parallaxes of 3 to 7 degrees.  NOISE is the pixel noise (standard deviation, both views)."""
import functools

import numpy as np

import mapinit_oracle as O

F = np.float32
INTR = np.array([500, 500, 320, 240], F)
NOISE = 0.1


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])


def project(P, R, t):
    Q = P @ R.T + t
    return np.stack([INTR[0] * Q[:, 0] / Q[:, 2] + INTR[2], INTR[1] * Q[:, 1] / Q[:, 2] + INTR[3]], 1)


def make_scene(seed, n, kind="general", outliers=0.0, extra=37, duplicates=0, t=(0.5, 0.05, 0.02), noise=NOISE, slope=(0.8, -0.5), behind=0, far=0):
    """n matches between two frames of n + extra keypoints each (the unmatched ones shift both normalisations), in shuffled order"""
    rng = np.random.default_rng(seed)
    R = rot(0.02, -0.05, 0.03)
    t = np.asarray(t, float)
    xy = rng.uniform([-2.2, -1.6], [2.2, 1.6], (n, 2))
    if kind == "plane":
        # the plane Z = 6 + a X + b Y met by the ray through (xy / 6, 1): P = (xy Z / 6, Z) with Z = 6 / (1 - (a x + b y) / 6)
        z = 6.0 / (1.0 - (slope[0] * xy[:, 0] + slope[1] * xy[:, 1]) / 6.0)
    else:
        z = rng.uniform(4.0, 8.0, n)
    P = np.concatenate([xy * (z[:, None] / 6.0), z[:, None]], 1)
    sd = np.full((n, 1), noise)
    if behind:   # the last `behind` points lie far BEHIND both cameras, noise-free: they obey the same epipolar geometry at almost no parallax
        P[n - behind:] = np.stack([np.linspace(-300, 300, behind), np.linspace(200, -200, behind), -np.linspace(1500, 3000, behind)], 1)
        sd[n - behind:] = 0
    if far:      # the last `far` points lie 100 to 3000 units deep: under 0.3 degrees of parallax, which excuses the depth tests for -t as for +t
        zf = np.exp(rng.uniform(np.log(100.0), np.log(3000.0), far))
        P[n - far:] = np.concatenate([xy[n - far:] * (zf[:, None] / 6.0), zf[:, None]], 1)
    p1 = project(P, np.eye(3), np.zeros(3)) + rng.normal(0, 1, (n, 2)) * sd
    p2 = project(P, R, t) + rng.normal(0, 1, (n, 2)) * sd
    n_out = int(round(outliers * n))
    if n_out:
        bad = rng.choice(n, n_out, replace=False)
        p2[bad] = rng.uniform([0, 0], [640, 480], (n_out, 2))
    kp1 = np.concatenate([p1, rng.uniform([0, 0], [640, 480], (extra, 2))]).astype(F)
    kp2 = np.concatenate([p2, rng.uniform([0, 0], [640, 480], (extra, 2))]).astype(F)
    perm1, perm2 = rng.permutation(n + extra), rng.permutation(n + extra)
    kp1s, kp2s = np.zeros_like(kp1), np.zeros_like(kp2)
    kp1s[perm1], kp2s[perm2] = kp1, kp2
    matches = np.stack([perm1[:n], perm2[:n]], 1).astype(np.int32)
    matches = matches[rng.permutation(n)]
    for d in range(duplicates):   # a second match onto an already matched reference keypoint
        matches[-1 - d, 0] = matches[d, 0]
    return dict(intr=INTR, kp1=kp1s, kp2=kp2s, matches=matches, R=R, t=t / max(np.linalg.norm(t), 1e-30), zrange=(float(z.min()), float(z.max())), kw={}, noise=noise,
                P=P, plane=(np.array([-slope[0], -slope[1], 1.0]), 6.0) if kind == "plane" else None)


def _with(sc, **kw):
    sc["kw"] = kw
    return sc


# a plane and a motion for which the two physically possible decompositions differ in their counts (most do not: the reference
# then refuses on the 0.75 rule, which plane_ambiguous_257 shows)
PLANE = dict(slope=(-0.57, -0.8), t=(0.49, 0.08, 0.02))
# name -> (builder, what must come out: model / ok, or None where the scene only has to agree)
SCENES = {
    "general_1000": (lambda: make_scene(1, 1000), dict(model=O.FUNDAMENTAL, ok=1)),
    "plane_1000": (lambda: make_scene(2, 1000, "plane", **PLANE), dict(model=O.HOMOGRAPHY, ok=1)),
    "general_outliers_257": (lambda: make_scene(3, 257, outliers=0.3), dict(model=O.FUNDAMENTAL)),
    "plane_outliers_257": (lambda: make_scene(4, 257, "plane", outliers=0.3, **PLANE), dict(model=O.HOMOGRAPHY)),
    "plane_ambiguous_257": (lambda: make_scene(16, 257, "plane", slope=(0.25, -0.15)), dict(model=O.HOMOGRAPHY, ok=0, rule075=True)),
    # 71 points 4 to 8 units deep and 186 far ones: (R, t) counts all 257, (R, -t) the 186 that low parallax excuses, 186 > 0.7 * 257.
    # sigma = 0.5 so that the far points' 0 to 2.5 pixels of disparity cost a homography enough for RH to stay under 0.40
    "similar_f_257": (lambda: _with(make_scene(20, 257, far=186), sigma=0.5), dict(model=O.FUNDAMENTAL, ok=0, rule07=True)),
    "pure_rotation_129": (lambda: make_scene(5, 129, t=(0.0, 0.0, 0.0)), dict(ok=0)),
    "duplicates_129": (lambda: make_scene(6, 129, duplicates=5), dict(model=O.FUNDAMENTAL, ok=1)),
    "behind_low_parallax_129": (lambda: make_scene(19, 129, behind=6), dict(model=O.FUNDAMENTAL, ok=1, behind=True)),
    "n8_it1": (lambda: _with(make_scene(31, 8), min_matches=8, iterations=1), None),
    "n9_it3": (lambda: _with(make_scene(31, 9), min_matches=8, iterations=3), None),
    "n63_it4": (lambda: _with(make_scene(9, 63), min_matches=8, iterations=4), None),
    "n64_it5": (lambda: _with(make_scene(10, 64), min_matches=8, iterations=5), None),
    "n65": (lambda: _with(make_scene(11, 65), min_matches=8), None),
    "good50": (lambda: _with(make_scene(12, 50, noise=0.05), min_triangulated=40), dict(ok=1, n_good=50)),
    "good51": (lambda: _with(make_scene(13, 51, noise=0.05), min_triangulated=40), dict(ok=1, n_good=51)),
    "good52": (lambda: _with(make_scene(14, 52, noise=0.05), min_triangulated=40), dict(ok=1, n_good=52)),
    "n49_defaults": (lambda: make_scene(15, 49), dict(ok=0, model=O.NONE)),
}
# scenes whose counted matches include low-parallax ones by construction: a cosine of 0.99998 or more lies within 1e-4 of that threshold
# by its nature, so there the winner's band cases are exactly its low-parallax matches, and runs are held to the oracle's states all the same
LOW_PARALLAX = ("similar_f_257", "pure_rotation_129", "behind_low_parallax_129")
MAX_EXEMPT, MAX_BAND = 0.10, 0.01
COND_EXEMPT = 1e8


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name][0]()


@functools.lru_cache(maxsize=None)
def oracle(name):
    sc = scene(name)
    return O.initialize(sc["intr"], sc["kp1"], sc["kp2"], sc["matches"], **sc["kw"])


def exempt_and_bands(r):
    """(exempt [2][iters] bool, band fraction over (hypothesis, match) pairs, whether a winner is exempt or a decision sits in a band)"""
    if "hyps" not in r:
        return np.zeros((2, 0), bool), 0.0, False
    ex = np.array([[h["cond"] > COND_EXEMPT for h in hs] for hs in r["hyps"]])
    band = np.mean([h["band"].mean() for hs in r["hyps"] for h in hs])
    tainted = bool((r["best_h"] >= 0 and ex[0][r["best_h"]]) or (r["best_f"] >= 0 and ex[1][r["best_f"]]) or r.get("ratio_band", False))
    return ex, float(band), tainted


def pose_bar(sc):
    """(rotation bar, translation-direction bar) in radians: how far the recovered pose may lie from the planted one, from the scene's pixel
    noise and the stage's own acceptance thresholds.  The pose is that of ONE unrefined 8-point hypothesis which the stage accepted
    because more than 90 % of the matches reproject within sqrt(th2) = 2 sigma pixels in both views; with three standard deviations of
    noise on the measured pixel the true projection may lie e = 2 + 3 noise pixels from the reprojection (the scene's own noise).  A rotation error d moves every
    image point by about f d pixels; a change of the translation direction can take that back only at one depth, since its image motion is
    proportional to 1 / Z, and leaves f d rel uncompensated at the ends of the depth range, rel = (Zmax - Zmin) / (Zmax + Zmin).  So
    f d rel <= e.  A translation-direction error dt moves a point by f dt b / Z pixels (b = 0.5 the baseline), which a rotation within its
    bar and the threshold together can hide: f dt b / Zmax <= f d + e."""
    e = 2.0 + 3 * sc["noise"]
    f = float(INTR[0])
    zmin, zmax = sc["zrange"]
    d = e / (f * (zmax - zmin) / (zmax + zmin))
    return d, (f * d + e) / (f * 0.5 / zmax)


def pose_error(R, t, sc):
    """(angle of R against the planted rotation, angle of t against the planted direction) in radians"""
    dR = np.asarray(R, float) @ sc["R"].T
    a = np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1))
    tt = np.asarray(t, float)
    return a, np.arccos(np.clip(tt @ sc["t"] / np.linalg.norm(tt), -1, 1))


@functools.lru_cache(maxsize=None)
def planted_non_finite():
    """A non-finite triangulation, which no keypoint input reaches (an inf coordinate is rejected by both models' chi-square tests or
    turns the score into NaN, and spoils the frame's normalisation): the reconstruction alone on the winning F21 of duplicates_129 with
    every match marked an inlier, after two coordinates are set to inf.  Match 128 shares its reference keypoint with match 0: the
    keypoint's flag, set by match 0, is CLEARED by the non-finite match 128, and both leave the survivors.  Match 50 is non-finite on the
    reference side.  -> (scene, model, M, mask, oracle result)"""
    base, r0 = scene("duplicates_129"), oracle("duplicates_129")
    sc = dict(base, kp1=base["kp1"].copy(), kp2=base["kp2"].copy())
    m = sc["matches"]
    assert m[128, 0] == m[0, 0] and r0["state"][0] == O.COUNTED_GOOD
    sc["kp2"][m[128, 1], 0] = np.inf
    sc["kp1"][m[50, 0], 1] = -np.inf
    M, mask = r0["hyps"][1][r0["best_f"]]["Mf"], np.ones(len(m), bool)
    res = O.empty_result(len(sc["kp1"]), len(m))
    res.update(model=O.FUNDAMENTAL, best_f=0, rh=F(0))
    r = O.reconstruct(res, sc["intr"], sc["kp1"], sc["kp2"], m, O.FUNDAMENTAL, M, mask, F(0))
    return sc, O.FUNDAMENTAL, M, mask, r
