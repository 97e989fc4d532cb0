"""CPU checks of the tracker oracle (oracle/track_oracle.cpp: system.cpp:6559-6954 on a map held by id) and of the stereo pose-only
solve it uses (oracle_pnp_solve_stereo against the real g2o's fixture).  The scenes stand on oracle_orb_extract keypoints; the camera
has no distortion, so the undistorted keypoints are the keypoints."""
import numpy as np
import pytest

import oracle_lib
import stereo_synth
import synth
import track_scenes as TS
from test_pnp_stereo import POSE_TOL, _golden


@pytest.fixture(scope="module")
def kpts(oracle):
    return oracle_lib.orb_extract(oracle, synth.frame(TS.W, TS.H, seed=5), 2000, 8, 1.2)


def _track(L, sc, **kw):
    return oracle_lib.track_pose(L, sc["fr"], sc["table"], sc["prev"], sc["local_ids"], sc["pose0"], **kw)


def _pnp_by_id(L, sc, m, pose, depth=None):
    """One oracle_pnp_solve over a match list, every look-up by map-point id in the table (pnpsolver.cpp:199-232)."""
    t = sc["table"]
    row_of_id = {int(v): i for i, v in enumerate(t["ids"])}
    r = np.array([row_of_id[int(v)] for v in m["trainIdx"]], np.int64)
    q = m["queryIdx"]
    kp = sc["fr"]["und_kpts"]
    pr = dict(n=len(m), pose=np.ascontiguousarray(pose, np.float32), intr=TS.INTR, p3d=np.ascontiguousarray(t["pos3d"][r].reshape(-1, 3)),
              kp=np.ascontiguousarray(np.stack([kp["x"][q], kp["y"][q]], 1).reshape(-1, 2)), invsig=np.ascontiguousarray(TS.INV_SF[kp["octave"][q]]),
              weight=np.where(t["stable"][r] != 0, np.float32(1), np.float32(0.5)).astype(np.float32))
    return oracle_lib.pnp_solve(L, pr) if depth is None else oracle_lib.pnp_solve_stereo(L, pr, depth[q], TS.BL)


# ------------------------------------------------------------------------------------------------ the stereo solve
@pytest.mark.parametrize("name", list(stereo_synth.CASES))
def test_oracle_stereo_pnp_matches_real_g2o(oracle, name):
    g = _golden()
    pr = stereo_synth.stereo_pnp_problem(**stereo_synth.CASES[name])
    got = oracle_lib.pnp_solve_stereo(oracle, pr, pr["depth"], pr["bl"])
    assert got["iters"].tolist() == g[f"{name}_iters"].tolist()
    assert got["ngood"] == int(g[f"{name}_ngood"])
    np.testing.assert_array_equal(got["bad"], g[f"{name}_bad"])
    assert np.abs(got["state"] - g[f"{name}_state"]).max() < POSE_TOL
    assert np.abs(got["pose"] - g[f"{name}_pose"]).max() < 1e-5
    if name == "mono600":   # all depths <= 0: the monocular solve itself, bit for bit (and so without depths)
        mono = oracle_lib.pnp_solve(oracle, pr)
        for d in (pr["depth"], None):
            s = oracle_lib.pnp_solve_stereo(oracle, pr, d, pr["bl"])
            for k in ("pose", "bad", "iters", "state"):
                assert s[k].tobytes() == mono[k].tobytes(), k
            assert s["ngood"] == mono["ngood"]


# ------------------------------------------------------------------------------------------------ the tracker's control flow
def test_oracle_lost_branch_is_one_search_and_one_solve(oracle, kpts):
    """Lost (too few matches, or too few inliers): the map search runs over every local-map candidate from pose0 with the wide radius, and
    the second solve over its matches alone starts from pose0."""
    cases = [(TS.scene(*kpts, 8, pose_noise=0.8), {}), (TS.scene(*kpts, 5), dict(min_inliers=100000)),
             (TS.with_first_search(oracle, TS.scene(*kpts, 21, n_prev=200, n_map=1500, uv_noise=0.3), 42, 12, seed=30)[0], {})]
    for sc, extra in cases:
        o = _track(oracle, sc, **extra)
        assert not o["tracked"]
        t = sc["table"]
        row_of_id = {int(v): i for i, v in enumerate(t["ids"])}
        lr = np.array([row_of_id[int(v)] for v in sc["local_ids"]], np.int64)
        mp = {k: np.ascontiguousarray(t[k][lr]) for k in ("ids", "pos3d", "normal", "min_dist", "max_dist", "desc")}
        m = oracle_lib.proj_match(oracle, sc["fr"], mp, sc["pose0"], 100.0, 15.0)["matches"]
        assert len(m) > 100
        assert o["matches_map"].tobytes() == m.tobytes() and o["matches_all"].tobytes() == m.tobytes()
        s = _pnp_by_id(oracle, sc, m, sc["pose0"])
        assert o["pose2"].tobytes() == s["pose"].tobytes() and o["inliers2"] == s["ngood"]
        np.testing.assert_array_equal(o["iters2"], s["iters"])
        np.testing.assert_array_equal(o["bad_all"], s["bad"])
        if len(o["matches_prev"]) > extra.get("min_inliers", 30):   # the first solve ran (its result is reported), the pose did not follow it
            assert o["inliers1"] == 30 and o["bad_prev"].sum() == 12
            s1 = _pnp_by_id(oracle, sc, o["matches_prev"], sc["pose0"])
            assert o["pose1"].tobytes() == s1["pose"].tobytes() != sc["pose0"].tobytes()
        else:       # too few matches: no first solve (the fallback found nothing)
            assert o["inliers1"] == 0 and o["iters1"].tolist() == [0] * 4 and not o["bad_prev"].any() and o["pose1"].tobytes() == sc["pose0"].tobytes()


def _check_union(o):
    """Tracked: every first-search match enters the union (an outlier too) — it survives the filter unless a map match of the same keypoint
    is strictly closer — and no map point the first search matched is matched again by the map search."""
    assert o["tracked"]
    m1, mm, ma = o["matches_prev"], o["matches_map"], o["matches_all"]
    ids1 = set(m1["trainIdx"].tolist())
    assert not (set(mm["trainIdx"].tolist()) & ids1)
    pairs = set(zip(ma["queryIdx"].tolist(), ma["trainIdx"].tolist()))
    best_map = {}
    for q, d in zip(mm["queryIdx"].tolist(), mm["distance"].tolist()):
        best_map[q] = min(d, best_map.get(q, np.inf))
    for q, tr, d in zip(m1["queryIdx"].tolist(), m1["trainIdx"].tolist(), m1["distance"].tolist()):
        assert (q, tr) in pairs or best_map.get(q, np.inf) < d, (q, tr)
    for q, tr in pairs:
        if tr in ids1:
            assert (q, tr) in set(zip(m1["queryIdx"].tolist(), m1["trainIdx"].tolist()))


def test_oracle_union_keeps_first_search_and_excludes_its_points(oracle, kpts):
    sc = TS.scene(*kpts, 31, n_prev=500, n_map=2500, uv_noise=0.3)
    sc, out = TS.with_first_search(oracle, sc, 160, 20, octave0_outliers=False, seed=31)
    o = _track(oracle, sc)
    _check_union(o)
    bad_ids = set(o["matches_prev"]["trainIdx"][o["bad_prev"] != 0].tolist())
    assert bad_ids == out, (sorted(bad_ids), sorted(out))
    # outliers of the first solve reach the second (the others lost their keypoint to a closer map match: _check_union)
    assert len(bad_ids & set(o["matches_all"]["trainIdx"].tolist())) >= len(bad_ids) // 2
    # half or more of the first-search matches are local-map candidates: the exclusion has something to exclude
    local = set(sc["local_ids"].tolist())
    assert np.mean([int(v) in local for v in o["matches_prev"]["trainIdx"]]) >= 0.5
    # the same control flow without the exclusion would have matched some of those points again
    lost = _track(oracle, sc, min_inliers=100000)
    again = set(lost["matches_map"]["trainIdx"].tolist()) & set(o["matches_prev"]["trainIdx"].tolist())
    assert again
    for seed in (5, 11):
        _check_union(_track(oracle, TS.scene(*kpts, seed, **(dict(n_prev=1500, n_map=6500) if seed == 11 else {}))))


@pytest.mark.parametrize("n_match, tracked", [(30, False), (31, True)])
def test_oracle_first_search_count_boundary(oracle, kpts, n_match, tracked):
    sc, _ = TS.with_first_search(oracle, TS.scene(*kpts, 21, n_prev=200, n_map=1500, uv_noise=0.3), n_match, 0, seed=n_match)
    o = _track(oracle, sc)
    assert len(o["matches_prev"]) == n_match
    assert o["tracked"] == tracked
    if tracked:
        assert o["inliers1"] == n_match and not o["bad_prev"].any()
    else:   # no first solve at exactly 30 matches
        assert o["inliers1"] == 0 and o["iters1"].tolist() == [0, 0, 0, 0] and o["pose1"].tobytes() == sc["pose0"].tobytes()
        assert len(o["matches_all"]) == len(o["matches_map"])


@pytest.mark.parametrize("n_inliers, tracked", [(29, False), (30, False), (31, True)])
def test_oracle_inlier_count_boundary(oracle, kpts, n_inliers, tracked):
    n_match = 42
    sc, out = TS.with_first_search(oracle, TS.scene(*kpts, 21, n_prev=200, n_map=1500, uv_noise=0.3), n_match, n_match - n_inliers, seed=n_inliers)
    o = _track(oracle, sc)
    assert len(o["matches_prev"]) == n_match >= 40
    assert o["inliers1"] == n_inliers, o["inliers1"]
    assert set(o["matches_prev"]["trainIdx"][o["bad_prev"] != 0].tolist()) == out
    assert o["tracked"] == tracked
    if tracked:
        assert len(o["matches_all"]) > len(o["matches_map"])
    else:
        assert o["matches_all"].tobytes() == o["matches_map"].tobytes()


def test_oracle_pose_for_map_continues_from_the_given_pose(oracle, kpts):
    sc = TS.scene(*kpts, 5)
    o = _track(oracle, sc)
    same = _track(oracle, sc, pose_for_map=o["pose1"])
    for k in o:
        assert np.asarray(o[k]).tobytes() == np.asarray(same[k]).tobytes(), k
    nudged = o["pose1"].copy()
    nudged[3] += np.float32(0.05)
    moved = _track(oracle, sc, pose_for_map=nudged)
    assert moved["matches_prev"].tobytes() == o["matches_prev"].tobytes() and moved["pose1"].tobytes() == o["pose1"].tobytes()
    assert moved["pose2"].tobytes() != o["pose2"].tobytes()


def test_oracle_stereo_uses_depth_in_both_solves(oracle, kpts):
    sc = TS.scene(*kpts, 5)
    dep = TS.depths(sc, 5)
    assert 0.4 < (dep > 0).mean() < 0.8
    o = _track(oracle, sc, depth=dep, bl=TS.BL)
    assert o["tracked"]
    s = _pnp_by_id(oracle, sc, o["matches_all"], o["pose1"], depth=dep)
    assert o["pose2"].tobytes() == s["pose"].tobytes() and o["inliers2"] == s["ngood"]
    mono = _track(oracle, sc)
    assert mono["pose2"].tobytes() != o["pose2"].tobytes()
    none = _track(oracle, sc, depth=np.zeros(len(dep), np.float32), bl=TS.BL)
    for k in mono:
        assert np.asarray(mono[k]).tobytes() == np.asarray(none[k]).tobytes(), k


def test_oracle_empty_inputs(oracle, kpts):
    sc = TS.scene(*kpts, 5, n_prev=0, n_map=800)
    o = _track(oracle, sc)
    assert len(o["matches_prev"]) == 0 and not o["tracked"] and len(o["matches_map"]) > 0
    sc = TS.scene(*kpts, 5, n_prev=300, n_map=800)
    sc["local_ids"] = sc["local_ids"][:0]
    o = _track(oracle, sc)
    assert o["tracked"] and len(o["matches_map"]) == 0 and o["matches_all"].tobytes() == o["matches_prev"].tobytes()
    sc = TS.scene(*kpts, 5, n_prev=200, n_map=500)
    sc["fr"] = TS.frame(np.zeros(0, oracle_lib.KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8))
    o = _track(oracle, sc)
    assert not o["tracked"] and len(o["matches_all"]) == 0 and o["pose2"].tobytes() == sc["pose0"].tobytes()


# ------------------------------------------------------------------------------------------------ another camera than the default one
def test_scene_camera_argument_leaves_the_default_scene_unchanged(kpts):
    a, b = TS.scene(*kpts, 5), TS.scene(*kpts, 5, intr=(TS.FX, TS.FY, TS.CX, TS.CY))
    for part in ("table", "prev", "fr"):
        for k in a[part]:
            assert np.asarray(a[part][k]).tobytes() == np.asarray(b[part][k]).tobytes(), (part, k)
    assert a["pose0"].tobytes() == b["pose0"].tobytes() and a["intr"].tobytes() == TS.INTR.tobytes()
    assert TS.depths(a, 5).tobytes() == TS.depths(b, 5, intr=(TS.FX, TS.FY, TS.CX, TS.CY)).tobytes()


@pytest.mark.parametrize("stereo", [False, True], ids=["mono", "stereo"])
def test_oracle_on_an_anisotropic_camera_notices_swapped_focal_lengths(oracle, kpts, stereo):
    """The scene the GPU tests compare on (TS.ANISO, fx != fy, principal point elsewhere) proves something only if the answer depends on
    which focal length is which: the same scene with fx and fy swapped in the frame gives other matches and another pose."""
    sc = TS.scene(*kpts, 41, intr=TS.ANISO)
    assert sc["fr"]["fx"] != sc["fr"]["fy"] and sc["intr"].tolist() == np.array(TS.ANISO, np.float32).tolist()
    dep = TS.depths(sc, 41) if stereo else None
    if stereo:
        assert 0.4 < (dep > 0).mean() < 0.8
    o = _track(oracle, sc, depth=dep, bl=TS.BL)
    assert o["tracked"] and o["inliers1"] > 100 and o["inliers2"] > 100
    sw = dict(sc)
    sw["fr"] = dict(sc["fr"], fx=sc["fr"]["fy"], fy=sc["fr"]["fx"])
    w = _track(oracle, sw, depth=dep, bl=TS.BL)
    assert w["matches_prev"].tobytes() != o["matches_prev"].tobytes() and w["matches_all"].tobytes() != o["matches_all"].tobytes()
    assert np.abs(w["pose2"] - o["pose2"]).max() > 1e-3 or not w["tracked"]     # (the comparison's pose tolerance is 1e-5)
    assert w["inliers2"] != o["inliers2"]
