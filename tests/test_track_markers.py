"""uh_track_pose_markers: the one-call tracker whose two solves also see the frame's markers, against the operators one after the other in
reference order (uh_projmatch_match_prev -> look-ups -> uh_pnp_solve_markers -> uh_projmatch_match -> exclusion, union, uh_filter_ambiguous
-> look-ups -> uh_pnp_solve_markers), bit for bit, on scenes of tests/track_scenes.py, monocular and stereo."""
import numpy as np
import pytest

import marker_synth
import track_scenes as TS
from test_track import _map_matches, _same
from test_track_oracle_gpu import _frame


def _markers(seed, n=2):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = TS.R0, TS.T0
    return marker_synth.make_markers(np.random.default_rng(30_000 + seed), T, TS.INTR, n)


def _sequence(F, sc, h, pnp, depth, prev_weight, markers, min_inliers=30, d1=75.0, r1=15.0, d2=100.0, rt=4.0, rl=15.0):
    """The operators one after the other with the host's list handling and look-ups in between; the same markers in both solves; the first
    solve only with MORE than min_inliers matches (system.cpp:6595), markers or not."""
    from ucoslam_cv3_amd._lib import lib, np_ptr
    from ucoslam_cv3_amd.projmatch import DMATCH_DTYPE

    pm, prev, mp, ukp, row_of, wmap = F["pm"], h["prev"], h["mp"], F["ukp"], h["prev_row"], h["map_weight"]
    dkw = (lambda q: {}) if depth is None else (lambda q: dict(depth=depth[q], bl=TS.BL))
    a = pm.matchFrameToPrevFrame(sc["pose0"], prev["ids"], prev["pos3d"], prev["octave"], prev["desc"], d1, r1)
    m1 = a["matches"]
    pid_to_i = {int(v): i for i, v in enumerate(prev["ids"])}
    it1 = np.array([pid_to_i[int(t)] for t in m1["trainIdx"]], np.int64)
    q1 = m1["queryIdx"]
    w1 = np.array([wmap[row_of[i]] if row_of[i] >= 0 else (1.0 if prev_weight is None else prev_weight[i]) for i in it1], np.float32)
    if len(m1) > min_inliers:
        s1 = pnp.solvePnp(sc["pose0"], sc["intr"], prev["pos3d"][it1].reshape(-1, 3), np.stack([ukp["x"][q1], ukp["y"][q1]], 1).reshape(-1, 2),
                          TS.INV_SF[ukp["octave"][q1]], w1, markers=markers, **dkw(q1))
    else:
        s1 = dict(ngood=0, pose=sc["pose0"], bad=np.zeros(len(m1), np.uint8), iters=np.zeros(4, np.int32))
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
            p3d[i] = mp["pos3d"][row]; w[i] = wmap[row]
        else:
            p3d[i] = prev["pos3d"][pid_to_i[int(tr)]]
            if prev_weight is not None:
                w[i] = prev_weight[pid_to_i[int(tr)]]
    qa = union["queryIdx"]
    s2 = pnp.solvePnp(pose_map, sc["intr"], p3d, np.stack([ukp["x"][qa], ukp["y"][qa]], 1).reshape(-1, 2), TS.INV_SF[ukp["octave"][qa]], w, markers=markers, **dkw(qa))
    return dict(matches_prev=m1, bad_prev=s1["bad"][: len(m1)], inliers1=s1["ngood"], iters1=s1["iters"], pose1=s1["pose"], tracked=bool(tracked), matches_map=m2,
                matches_all=union, bad_all=s2["bad"][: len(union)], inliers2=s2["ngood"], iters2=s2["iters"], pose2=s2["pose"])


def _fused(F, sc, h, pnp, markers, depth=None, prev_weight=None, **kw):
    return F["pm"].trackPoseMarkers(pnp, sc["pose0"], sc["intr"], TS.INV_SF, h["prev"], h["mp"], markers=markers, depth=depth, bl=TS.BL if depth is not None else 0.0,
                                    prev_weight=prev_weight, prev_map_row=h["prev_row"], map_weight=h["map_weight"], **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["mono", "stereo"])
def test_track_pose_markers_equals_the_operators_in_reference_order(hip_ctx, mode):
    from ucoslam_cv3_amd.pnp import PnPSolver

    pnp = PnPSolver(hip_ctx)
    for seed, kw in ((5, {}), (7, dict(n_prev=300, n_map=1200))):
        F = _frame(hip_ctx, seed)
        sc = TS.scene(F["ukp"], F["desc"], seed, stable_outside=(mode == "mono"), **kw)
        h = TS.hip_inputs(sc)
        depth = TS.depths(sc, seed) if mode == "stereo" else None
        pw = h["prev_weight"] if mode == "stereo" else None
        mk = _markers(seed)
        f = _fused(F, sc, h, pnp, mk, depth, pw)
        _same(f, _sequence(F, sc, h, pnp, depth, pw, mk), f"{mode} seed {seed}")
        assert f["tracked"] and f["inliers2"] > 100
        # the markers are in both solves: without them the solves differ
        g = _fused(F, sc, h, pnp, None, depth, pw)
        assert any(np.asarray(f[k]).tobytes() != np.asarray(g[k]).tobytes() for k in ("pose1", "pose2", "iters1", "iters2")), (mode, seed)


@pytest.mark.gpu
def test_track_pose_markers_without_markers_equals_track_pose_stereo(hip_ctx):
    from ucoslam_cv3_amd.pnp import PnPSolver

    pnp = PnPSolver(hip_ctx)
    F = _frame(hip_ctx, 5)
    sc = TS.scene(F["ukp"], F["desc"], 5)
    h = TS.hip_inputs(sc)
    depth = TS.depths(sc, 5)
    base = F["pm"].trackPoseStereo(pnp, sc["pose0"], sc["intr"], TS.INV_SF, h["prev"], h["mp"], depth=depth, bl=TS.BL, prev_weight=h["prev_weight"],
                                   prev_map_row=h["prev_row"], map_weight=h["map_weight"])
    empty = dict(pose_g2m=np.zeros((0, 16), np.float32), size=np.zeros(0, np.float32), und_corners=np.zeros((0, 8), np.float32))
    for mk in (None, empty):
        got = _fused(F, sc, h, pnp, mk, depth, h["prev_weight"])
        _same(got, base, "no markers")
        assert got["pose1"].tobytes() == base["pose1"].tobytes()
    mono = F["pm"].trackPose(pnp, sc["pose0"], sc["intr"], TS.INV_SF, h["prev"], h["mp"], prev_map_row=h["prev_row"], map_weight=h["map_weight"])
    _same(_fused(F, sc, h, pnp, None), mono, "no markers, no stereo")


@pytest.mark.gpu
def test_track_pose_markers_reports_no_first_solve_with_few_matches(hip_ctx):
    """n_prev <= min_inliers: no first solve is reported even with markers (pose0, no iterations, no flags); the second solve has them."""
    from ucoslam_cv3_amd._lib import UcoslamHipError
    from ucoslam_cv3_amd.pnp import PnPSolver

    pnp = PnPSolver(hip_ctx)
    F = _frame(hip_ctx, 9)
    sc = TS.scene(F["ukp"], F["desc"], 9, stable_outside=True)
    h = TS.hip_inputs(sc)
    mk = _markers(9)
    f = _fused(F, sc, h, pnp, mk, min_inliers=100000)
    assert len(f["matches_prev"]) > 100 and not f["tracked"] and f["inliers1"] == 0 and f["iters1"].tolist() == [0, 0, 0, 0]
    assert f["pose1"].tobytes() == sc["pose0"].tobytes() and not f["bad_prev"].any()
    assert all(v > 0 for v in f["iters2"])
    _same(f, _sequence(F, sc, h, pnp, None, None, mk, min_inliers=100000), "few matches")
    bad = dict(mk, size=np.array([0.2, 0.0], np.float32))
    with pytest.raises(UcoslamHipError):
        _fused(F, sc, h, pnp, bad)
