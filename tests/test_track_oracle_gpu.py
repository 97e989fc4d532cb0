"""uh_track_pose and uh_track_pose_stereo (csrc/track.hpp) against the CPU oracle of the tracker's control flow (oracle/track_oracle.cpp,
system.cpp:6559-6954 on a map held by id).  The scenes are reference-consistent (tests/track_scenes.py): one position and one stability
per map-point id, the fused call's inputs derived from that table.

Comparison: the first search, the first solve's flags, iterations and inlier count and the decision exactly, its pose within 1e-5.  The
oracle then runs again from the map search onward at the fused call's float pose (pose_for_map), so that one ulp of the first pose cannot
move a candidate across a search radius; against that run the map search, the union and the second solve's flags, iterations and inlier
count exactly, its pose within 1e-5.  When both first poses are bit-equal the rerun must change nothing."""
import numpy as np
import pytest

import oracle_lib
import synth
import track_scenes as TS

POSE_TOL = 1e-5
MODES = ["mono", "stereo_prev_weight", "stereo_depth", "stereo_no_depth"]


def _frame(hip_ctx, seed, blank=False, intr=None):
    from ucoslam_cv3_amd.orb import Camera, DeviceFrame, FeatParams, ORBextractor
    from ucoslam_cv3_amd.projmatch import ProjectionMatcher

    fx, fy, cx, cy = (TS.FX, TS.FY, TS.CX, TS.CY) if intr is None else intr
    ext = ORBextractor(hip_ctx)
    ext.setCamera(Camera(fx, fy, cx, cy, ()))
    fr = DeviceFrame(hip_ctx).setTreeBuilder(False)
    img = np.full((TS.H, TS.W), 90, np.uint8) if blank else synth.frame(TS.W, TS.H, seed=seed)
    kps, desc, und = ext.extractFrameDev(img, fr, FeatParams(maxFeatures=2000, nOctaveLevels=8, scaleFactor=1.2))
    ukp = kps.copy()
    ukp["x"], ukp["y"] = und[:, 0], und[:, 1]
    pm = ProjectionMatcher(hip_ctx)
    pm.setFrameDev(fr, TS.SF, fx, fy, cx, cy, (0, 0), (TS.W, TS.H), und_kpts=ukp)
    return dict(pm=pm, ukp=ukp, desc=np.ascontiguousarray(desc).reshape(-1, 32), keep=(ext, fr))


def _depth(sc, mode, seed):
    n = len(sc["fr"]["und_kpts"])
    if mode == "stereo_depth":
        d = TS.depths(sc, seed)
        assert n == 0 or 0.4 < (d > 0).mean() < 0.8
        return d
    if mode == "stereo_no_depth":
        return np.where(np.arange(n) % 2 == 0, np.float32(0), np.float32(-1)).astype(np.float32)
    return None


def _fused(F, pnp, sc, mode, depth, **kw):
    h = TS.hip_inputs(sc)
    if mode == "mono":
        assert all(sc["table"]["stable"][np.isin(sc["table"]["ids"], h["prev"]["ids"]) & ~np.isin(sc["table"]["ids"], sc["local_ids"])])
        return F["pm"].trackPose(pnp, sc["pose0"], sc["intr"], TS.INV_SF, h["prev"], h["mp"], prev_map_row=h["prev_row"], map_weight=h["map_weight"], **kw)
    return F["pm"].trackPoseStereo(pnp, sc["pose0"], sc["intr"], TS.INV_SF, h["prev"], h["mp"], depth=depth, bl=TS.BL, prev_weight=h["prev_weight"],
                                   prev_map_row=h["prev_row"], map_weight=h["map_weight"], **kw)


def _agree(L, sc, f, depth, what, **kw):
    """f (the fused call) against the oracle under the comparison rule of the module docstring; returns the oracle's first run."""
    o = oracle_lib.track_pose(L, sc["fr"], sc["table"], sc["prev"], sc["local_ids"], sc["pose0"], depth=depth, bl=TS.BL, **kw)
    assert f["matches_prev"].tobytes() == o["matches_prev"].tobytes(), (what, len(f["matches_prev"]), len(o["matches_prev"]))
    np.testing.assert_array_equal(f["bad_prev"], o["bad_prev"], err_msg=f"{what}: bad_prev")
    np.testing.assert_array_equal(f["iters1"], o["iters1"], err_msg=f"{what}: iters1")
    assert f["inliers1"] == o["inliers1"], (what, f["inliers1"], o["inliers1"])
    assert np.abs(f["pose1"] - o["pose1"]).max() < POSE_TOL, what
    assert f["tracked"] == o["tracked"], (what, f["tracked"], o["tracked"], o["inliers1"])
    o2 = oracle_lib.track_pose(L, sc["fr"], sc["table"], sc["prev"], sc["local_ids"], sc["pose0"], depth=depth, bl=TS.BL, pose_for_map=f["pose1"], **kw)
    if f["pose1"].tobytes() == o["pose1"].tobytes():
        for k in o:
            assert np.asarray(o[k]).tobytes() == np.asarray(o2[k]).tobytes(), (what, "rerun", k)
    for k in ("matches_map", "matches_all"):
        assert f[k].tobytes() == o2[k].tobytes(), (what, k, len(f[k]), len(o2[k]))
    np.testing.assert_array_equal(f["bad_all"], o2["bad_all"], err_msg=f"{what}: bad_all")
    np.testing.assert_array_equal(f["iters2"], o2["iters2"], err_msg=f"{what}: iters2")
    assert f["inliers2"] == o2["inliers2"], (what, f["inliers2"], o2["inliers2"])
    assert np.abs(f["pose2"] - o2["pose2"]).max() < POSE_TOL, what
    return o


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_fused_tracker_agrees_with_oracle(hip_ctx, oracle, mode):
    from ucoslam_cv3_amd.pnp import PnPSolver

    pnp = PnPSolver(hip_ctx)
    for seed, kw in ((5, {}), (6, {}), (7, dict(n_prev=300, n_map=1200)), (8, dict(pose_noise=0.8)), (11, dict(n_prev=1500, n_map=6500))):   # (the last: lists too long for LDS)
        F = _frame(hip_ctx, seed)
        sc = TS.scene(F["ukp"], F["desc"], seed, stable_outside=(mode == "mono"), **kw)
        if mode == "stereo_prev_weight":
            assert (TS.hip_inputs(sc)["prev_weight"] < 1).any()
        depth = _depth(sc, mode, seed)
        o = _agree(oracle, sc, _fused(F, pnp, sc, mode, depth), depth, f"{mode} seed {seed}")
        if not kw.get("pose_noise"):
            assert o["tracked"] and o["inliers2"] > 100, (seed, o["inliers1"], o["inliers2"])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_fused_tracker_lost_and_empty_agree_with_oracle(hip_ctx, oracle, mode):
    from ucoslam_cv3_amd.pnp import PnPSolver

    pnp = PnPSolver(hip_ctx)
    F = _frame(hip_ctx, 9)
    sc = TS.scene(F["ukp"], F["desc"], 9, stable_outside=True)
    d = _depth(sc, mode, 9)
    o = _agree(oracle, sc, _fused(F, pnp, sc, mode, d, min_inliers=100000), d, f"{mode} lost", min_inliers=100000)
    assert not o["tracked"] and len(o["matches_prev"]) > 100
    for n_prev, n_map in ((0, 1500), (600, 0)):
        sc = TS.scene(F["ukp"], F["desc"], 10 + n_prev, n_prev=n_prev, n_map=max(n_map, 700), stable_outside=True)
        if n_map == 0:   # (every previous-frame item is outside the local map now: stable, for the mono entry)
            sc["local_ids"] = sc["local_ids"][:0]
            sc["table"]["stable"][:] = 1
        _agree(oracle, sc, _fused(F, pnp, sc, mode, d), d, f"{mode} n_prev {n_prev} n_map {n_map}")
    B = _frame(hip_ctx, 5, blank=True)
    assert len(B["ukp"]) == 0
    sc = TS.scene(F["ukp"], F["desc"], 5, n_prev=200, n_map=500, stable_outside=True)
    sc["fr"] = TS.frame(B["ukp"], B["desc"])
    d0 = None if d is None else d[:0]
    o = _agree(oracle, sc, _fused(B, pnp, sc, mode, d0), d0, f"{mode} no keypoints")
    assert not o["tracked"] and len(o["matches_all"]) == 0


def _boundary(L, F, n_match, n_out, seed):
    sc = TS.scene(F["ukp"], F["desc"], 21, n_prev=200, n_map=1500, uv_noise=0.3, stable_outside=True)
    return TS.with_first_search(L, sc, n_match, n_out, seed=seed)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["mono", "stereo_prev_weight"])
def test_fused_tracker_decision_boundaries(hip_ctx, oracle, mode):
    """30 matches: no first solve, lost; 31 inliers of 31: tracked.  29 / 30 / 31 inliers of 42 matches: lost, lost, tracked (strict
    comparison, system.cpp:6595 / :6813).  Each scene asserts the count it was built for."""
    from ucoslam_cv3_amd.pnp import PnPSolver

    pnp = PnPSolver(hip_ctx)
    F = _frame(hip_ctx, 21)
    for n_match, n_in, tracked in ((30, 30, False), (31, 31, True), (42, 29, False), (42, 30, False), (42, 31, True)):
        sc, out = _boundary(oracle, F, n_match, n_match - n_in, seed=n_match * 100 + n_in)
        o = _agree(oracle, sc, _fused(F, pnp, sc, mode, None), None, f"{mode} {n_match} matches {n_in} inliers")
        assert len(o["matches_prev"]) == n_match and o["tracked"] == tracked
        assert o["inliers1"] == (n_in if n_match > 30 else 0)
        assert set(o["matches_prev"]["trainIdx"][o["bad_prev"] != 0].tolist()) == out


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_fused_tracker_first_solve_outliers_and_seen_points(hip_ctx, oracle, mode):
    """A tracked frame with >= 10 % first-solve outliers, >= half of the first search's points in the local map: the outliers enter the
    union, and the local-map search skips every point the first search matched."""
    from ucoslam_cv3_amd.pnp import PnPSolver

    pnp = PnPSolver(hip_ctx)
    F = _frame(hip_ctx, 31)
    sc = TS.scene(F["ukp"], F["desc"], 31, n_prev=500, n_map=2500, uv_noise=0.3, stable_outside=(mode == "mono"))
    sc, out = TS.with_first_search(oracle, sc, 160, 20, octave0_outliers=False, seed=31)
    d = _depth(sc, mode, 31)
    o = _agree(oracle, sc, _fused(F, pnp, sc, mode, d), d, f"{mode} outliers")
    assert o["tracked"] and o["bad_prev"].sum() >= 16
    local = set(sc["local_ids"].tolist())
    assert np.mean([int(v) in local for v in o["matches_prev"]["trainIdx"]]) >= 0.5
    assert set(o["matches_prev"]["trainIdx"][o["bad_prev"] != 0].tolist()) & set(o["matches_all"]["trainIdx"].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_fused_tracker_agrees_with_oracle_on_an_anisotropic_camera(hip_ctx, oracle, mode):
    """fx != fy and a principal point elsewhere (TS.ANISO): every other scene has fx == fy, where swapping the two in a projection or a
    Jacobian row changes nothing.  tests/test_track_oracle.py shows that the oracle's answer on this scene depends on which is which."""
    from ucoslam_cv3_amd.pnp import PnPSolver

    pnp = PnPSolver(hip_ctx)
    for seed, kw in ((41, {}), (42, dict(n_prev=1500, n_map=6500))):   # (the last: lists too long for LDS)
        F = _frame(hip_ctx, seed, intr=TS.ANISO)
        sc = TS.scene(F["ukp"], F["desc"], seed, stable_outside=(mode == "mono"), intr=TS.ANISO, **kw)
        assert sc["intr"][0] != sc["intr"][1]
        depth = _depth(sc, mode, seed)
        o = _agree(oracle, sc, _fused(F, pnp, sc, mode, depth), depth, f"aniso {mode} seed {seed}")
        assert o["tracked"] and o["inliers2"] > 100, (seed, o["inliers1"], o["inliers2"])
