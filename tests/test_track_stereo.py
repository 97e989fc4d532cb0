"""uh_track_pose_stereo: the one-call tracker with stereo / RGB-D depths and per-item previous-frame weights, against the operators
one after the other (uh_projmatch_match_prev -> look-ups -> uh_pnp_solve_stereo -> uh_projmatch_match -> union, uh_filter_ambiguous ->
look-ups -> uh_pnp_solve_stereo), bit for bit, with both kd-tree builders."""
import numpy as np
import pytest

from test_track import _first_solve, _map_matches, _same, _scene

BL = 0.54


def _depths(sc, seed, n_map=3000):
    """Per keypoint of the frame: the camera z of a map point _scene placed behind it (its draws of `pick` and `z` are the first of its
    generator) with 0.5 % noise, a grossly wrong depth for a few, none (0 or < 0) for about a third and for keypoints without a point."""
    rng = np.random.default_rng(seed)
    n = len(sc["ukp"])
    pick = rng.integers(0, n, n_map)
    z = rng.uniform(4, 40, n_map)
    depth = np.zeros(n, np.float64)
    depth[pick] = z
    r2 = np.random.default_rng(1000 + seed)
    depth *= 1 + r2.normal(0, 0.005, n)
    depth[r2.random(n) < 0.05] *= 2.5
    depth[r2.random(n) < 0.35] = 0.0
    depth[r2.random(n) < 0.02] = -1.0
    return depth.astype(np.float32)


def _sequence_stereo(sc, pnp, depth, prev_weight, min_inliers=30, d1=75.0, r1=15.0, d2=100.0, rt=4.0, rl=15.0):
    """The operators one after the other, with the host's list handling and look-ups in between (the stereo form of
    tests/test_track.py::_sequence): depth[queryIdx] per match in both solves; a previous-frame item's weight is map_weight[row] for
    row >= 0, else prev_weight[i] (or 1 without prev_weight), in both solves."""
    from ucoslam_cv3_amd._lib import lib, np_ptr
    from ucoslam_cv3_amd.projmatch import DMATCH_DTYPE

    pm, prev, mp, ukp = sc["pm"], sc["prev"], sc["mp"], sc["ukp"]
    row_of = sc["prev_row"]
    a = pm.matchFrameToPrevFrame(sc["pose0"], prev["ids"], prev["pos3d"], prev["octave"], prev["desc"], d1, r1)
    m1 = a["matches"]
    pid_to_i = {int(v): i for i, v in enumerate(prev["ids"])}
    it1 = np.array([pid_to_i[int(t)] for t in m1["trainIdx"]], np.int64)
    q1 = m1["queryIdx"]
    w1 = np.array([sc["weight"][row_of[i]] if row_of[i] >= 0 else (1.0 if prev_weight is None else prev_weight[i]) for i in it1], np.float32)
    s1 = _first_solve(pnp, sc, m1, prev["pos3d"][it1].reshape(-1, 3), w1, min_inliers, depth=depth[q1], bl=BL)
    tracked = s1["ngood"] > min_inliers
    pose_map = s1["pose"] if tracked else sc["pose0"]
    b = pm.matchFrameToMapPoints(pose_map, mp["ids"], mp["pos3d"], mp["normal"], mp["min_dist"], mp["max_dist"], mp["desc"], d2, rt if tracked else rl)
    rows1 = row_of[it1] if len(it1) else np.zeros(0, np.int32)
    m2 = _map_matches(b, mp["ids"], rows1[rows1 >= 0] if tracked else [])
    union = np.concatenate([m1 if tracked else m1[:0], m2]).astype(DMATCH_DTYPE)
    if len(union):
        union = np.ascontiguousarray(union)
        k = lib().uh_filter_ambiguous(np_ptr(union), len(union), 0)
        assert k >= 0
        union = union[:k]
    mid_to_row = {int(v): i for i, v in enumerate(mp["ids"])}
    p3d = np.zeros((len(union), 3), np.float32)
    w = np.ones(len(union), np.float32)
    for i, tr in enumerate(union["trainIdx"]):
        row = mid_to_row.get(int(tr), -1)
        if row >= 0:
            p3d[i] = mp["pos3d"][row]; w[i] = sc["weight"][row]
        else:
            p3d[i] = prev["pos3d"][pid_to_i[int(tr)]]
            if prev_weight is not None:
                w[i] = prev_weight[pid_to_i[int(tr)]]
    qa = union["queryIdx"]
    s2 = pnp.solvePnp(pose_map, sc["intr"], p3d, np.stack([ukp["x"][qa], ukp["y"][qa]], 1).reshape(-1, 2), sc["inv_sf"][ukp["octave"][qa]], w,
                      depth=depth[qa], bl=BL)
    return dict(matches_prev=m1, bad_prev=s1["bad"][: len(m1)], inliers1=s1["ngood"], iters1=s1["iters"], pose1=s1["pose"], tracked=bool(tracked), matches_map=m2,
                matches_all=union, bad_all=s2["bad"][: len(union)], inliers2=s2["ngood"], iters2=s2["iters"], pose2=s2["pose"])


def _prev_weight(sc, seed):
    rng = np.random.default_rng(100 + seed)
    return np.where(rng.random(len(sc["prev"]["ids"])) < 0.4, np.float32(0.5), np.float32(1.0)).astype(np.float32)


def _fused(sc, pnp, **kw):
    return sc["pm"].trackPoseStereo(pnp, sc["pose0"], sc["intr"], sc["inv_sf"], sc["prev"], sc["mp"], prev_map_row=sc["prev_row"], map_weight=sc["weight"], **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("host_tree", [False, True], ids=["device_tree", "host_tree"])
def test_track_pose_stereo_equals_the_operators_in_reference_order(hip_ctx, host_tree):
    from ucoslam_cv3_amd.pnp import PnPSolver

    pnp = PnPSolver(hip_ctx)
    for seed, kw in ((5, {}), (7, dict(n_prev=300, n_map=1200)), (8, dict(pose_noise=0.8)), (11, dict(n_prev=1500, n_map=6500))):
        sc = _scene(hip_ctx, seed, host_tree, **kw)
        depth = _depths(sc, seed, kw.get("n_map", 3000))
        assert (depth > 0).mean() > 0.2
        for pw in (None, _prev_weight(sc, seed)):
            s = _sequence_stereo(sc, pnp, depth, pw)
            f = _fused(sc, pnp, depth=depth, bl=BL, prev_weight=pw)
            _same(f, s, f"seed {seed} prev_weight {pw is not None}")
        if not kw.get("pose_noise"):
            assert f["tracked"] and f["inliers2"] > 30


@pytest.mark.gpu
def test_track_pose_stereo_without_depth_equals_track_pose(hip_ctx):
    from ucoslam_cv3_amd.pnp import PnPSolver

    pnp = PnPSolver(hip_ctx)
    for seed in (5, 8):
        sc = _scene(hip_ctx, seed, False, **(dict(pose_noise=0.8) if seed == 8 else {}))
        a = sc["pm"].trackPose(pnp, sc["pose0"], sc["intr"], sc["inv_sf"], sc["prev"], sc["mp"], prev_map_row=sc["prev_row"], map_weight=sc["weight"])
        b = _fused(sc, pnp)
        _same(b, a, f"seed {seed}")
        assert b["pose1"].tobytes() == a["pose1"].tobytes()


@pytest.mark.gpu
def test_track_pose_stereo_prev_weight_reaches_both_solves(hip_ctx):
    """A previous-frame item outside the local map weighs prev_weight[i] (not 1) in the solves, exactly as the operator sequence with the
    reference's per-edge weights.  (The robust weight scales the chi2 sums only, not the normal equations: it changes Levenberg's damping
    and stopping decisions, so some scene / weight pairs move the result and others leave it bit-identical — at least one must move.)"""
    from ucoslam_cv3_amd.pnp import PnPSolver

    pnp = PnPSolver(hip_ctx)
    moved = 0
    for seed, kw in ((5, {}), (8, dict(pose_noise=0.8)), (6, dict(pose_noise=0.3))):
        sc = _scene(hip_ctx, seed, False, **kw)
        assert (sc["prev_row"] < 0).any()
        base = _fused(sc, pnp)
        for wv in (0.5, 1e-3):
            pw = np.full(len(sc["prev"]["ids"]), np.float32(wv))
            got = _fused(sc, pnp, prev_weight=pw)
            _same(got, _sequence_stereo(sc, pnp, np.zeros(len(sc["ukp"]), np.float32), pw), f"seed {seed} prev_weight {wv}")
            moved += any(got[k].tobytes() != base[k].tobytes() for k in ("pose1", "pose2", "iters1", "iters2", "bad_prev", "bad_all"))
    assert moved > 0


@pytest.mark.gpu
def test_track_pose_stereo_refuses_bad_rows_and_baseline(hip_ctx):
    from ucoslam_cv3_amd._lib import UcoslamHipError
    from ucoslam_cv3_amd.pnp import PnPSolver

    pnp = PnPSolver(hip_ctx)
    sc = _scene(hip_ctx, 7, False, n_prev=300, n_map=1200)
    for bad_row in (len(sc["mp"]["ids"]), -2):
        rows = sc["prev_row"].copy()
        rows[len(rows) // 2] = bad_row
        with pytest.raises(UcoslamHipError):
            sc["pm"].trackPoseStereo(pnp, sc["pose0"], sc["intr"], sc["inv_sf"], sc["prev"], sc["mp"], prev_map_row=rows, map_weight=sc["weight"])
    with pytest.raises(UcoslamHipError):
        _fused(sc, pnp, depth=_depths(sc, 7, 1200), bl=0.0)
    _fused(sc, pnp, depth=_depths(sc, 7, 1200), bl=BL)   # the session is still usable


@pytest.mark.gpu
@pytest.mark.parametrize("host_tree", [False, True], ids=["device_tree", "host_tree"])
def test_track_pose_stereo_on_an_anisotropic_camera_agrees_with_oracle(hip_ctx, oracle, host_tree):
    """uh_track_pose_stereo with depths and previous-frame weights on a camera with fx != fy and its principal point elsewhere, against
    oracle_track_pose (every scene above has fx == fy), with both kd-tree builders.  Comparison rule and exact-equality assertions:
    tests/test_track_oracle_gpu.py::_agree."""
    import synth
    import track_scenes as TS
    from test_track_oracle_gpu import _agree
    from ucoslam_cv3_amd.orb import Camera, DeviceFrame, FeatParams, ORBextractor
    from ucoslam_cv3_amd.pnp import PnPSolver
    from ucoslam_cv3_amd.projmatch import ProjectionMatcher

    fx, fy, cx, cy = TS.ANISO
    pnp = PnPSolver(hip_ctx)
    ext = ORBextractor(hip_ctx)
    ext.setCamera(Camera(fx, fy, cx, cy, ()))
    fr = DeviceFrame(hip_ctx).setTreeBuilder(host_tree)
    kps, desc, und = ext.extractFrameDev(synth.frame(TS.W, TS.H, seed=43), fr, FeatParams(maxFeatures=2000, nOctaveLevels=8, scaleFactor=1.2))
    ukp = kps.copy()
    ukp["x"], ukp["y"] = und[:, 0], und[:, 1]
    pm = ProjectionMatcher(hip_ctx)
    pm.setFrameDev(fr, TS.SF, fx, fy, cx, cy, (0, 0), (TS.W, TS.H), und_kpts=ukp)
    sc = TS.scene(ukp, np.ascontiguousarray(desc).reshape(-1, 32), 43, intr=TS.ANISO)
    depth = TS.depths(sc, 43)
    assert 0.4 < (depth > 0).mean() < 0.8
    h = TS.hip_inputs(sc)
    assert (h["prev_weight"] < 1).any() and (h["prev_row"] < 0).any()
    f = pm.trackPoseStereo(pnp, sc["pose0"], sc["intr"], TS.INV_SF, h["prev"], h["mp"], depth=depth, bl=TS.BL, prev_weight=h["prev_weight"],
                           prev_map_row=h["prev_row"], map_weight=h["map_weight"])
    o = _agree(oracle, sc, f, depth, f"aniso stereo host_tree {host_tree}")
    assert o["tracked"] and o["inliers2"] > 100
