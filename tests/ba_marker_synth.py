"""Deterministic bundle-adjustment problems with squared planar markers (the inputs of tests/golden/ba_marker_golden.npz).

The keypoint part is stereo_ba_synth.stereo_ba_problem's (one camera) or het_ba_synth.het_ba_problem's (a camera per keyframe); on top
of it the map holds markers, each a free pose g2m (float 4x4, Marker::pose_g2m) with a side length, seen by a named list of keyframes:
one marker edge per (marker, frame) in the reference's order (markers ascending, within a marker its frames ascending:
globaloptimizer_g2o.cpp:320-352), und_corners = the projection of the four corners (Marker::get3DPointsLocalRefSystem's order) through
the true poses with pixel noise, as float.  edge_weight is frame_MarkerWeight of :281-299, restated here in Python from the problem's
own observations (frame_weights); frame_n_markers is frame.markers.size(), which also counts markers without a valid pose.

extra_frames keyframes are appended behind the keypoint problem's: they see no landmark and are fixed (the frames that join through a
marker, FIXED_WITHOUTPOINTS).  thin_frame = (k, n) leaves keyframe k with at most n observations (kpw <= 40: weight 1)."""
import numpy as np

import het_ba_synth
import stereo_ba_synth
import synth

INPUT_KEYS = stereo_ba_synth.INPUT_KEYS
MARKER_KEYS = ("mk_pose", "mk_size", "me_marker", "me_frame", "me_corners", "me_weight")
MARKERS_OPT_WEIGHT = float(np.float32(0.5))   # ParamSet::markersOptWeight, a float
MIN_MARKERS_FOR_MAX_WEIGHT = 5                # ParamSet::minMarkersForMaxWeight


# The keypoint side of every case but mk_hard: no outliers and a start close enough that no edge ever leaves the quadratic part of
# its Huber kernel, so the run does not depend on the kernel's width (see make_ba_marker_golden.py, condition 1) and ends after a few
# iterations (condition 2: every evaluation of a marker edge is a chance for a float rounding to flip)
QUIET = dict(outlier_frac=0.0, gross_frac=0.0, pose_noise=1e-3, point_noise=0.005, pix_noise=0.4)


def _rot(w):
    return synth._se3_exp(np.r_[w, 0, 0, 0])[:3, :3]


def frame_weights(K, obs_kf, obs_w, obs_depth, frame_n_markers):
    """frame_MarkerWeight (:281-299) per keyframe and the keypoint weight sums kpw it is computed from.  _InvScaleFactors is a
    vector<float>: an edge adds the FLOAT product 2 * f (two rows) or 3 * f (three rows) to the frame's double sum, in edge order."""
    kpw = np.zeros(K, np.float64)
    for k, w, d in zip(obs_kf, obs_w, obs_depth):
        kpw[k] += float(np.float32(3 if d > 0 else 2) * np.float32(w))
    weight = np.ones(K, np.float64)
    for k in range(K):
        n = int(frame_n_markers[k])
        if kpw[k] > 40 and n > 0:
            marker_perct = MARKERS_OPT_WEIGHT * min(1.0, float(n) / MIN_MARKERS_FOR_MAX_WEIGHT)
            weight[k] = (marker_perct * kpw[k]) / float(n * 8)
    return weight, kpw


def _drop_observations(pr, drop):
    """pr without the observations flagged in `drop`, without the landmarks that are left with fewer than two observers (one, where
    it has depth), renumbered."""
    keep = ~drop
    while True:
        cnt = np.bincount(pr["obs_pt"][keep], minlength=pr["P"])
        has_depth = np.bincount(pr["obs_pt"][keep], weights=(pr["obs_depth"][keep] > 0), minlength=pr["P"]) > 0
        lone = keep & (cnt[pr["obs_pt"]] < 2) & ~((cnt[pr["obs_pt"]] == 1) & has_depth[pr["obs_pt"]])
        if not lone.any():
            break
        keep &= ~lone
    alive = np.bincount(pr["obs_pt"][keep], minlength=pr["P"]) > 0
    remap = -np.ones(pr["P"], np.int32)
    remap[alive] = np.arange(alive.sum(), dtype=np.int32)
    out = dict(pr)
    out.update(P=int(alive.sum()), E=int(keep.sum()), points=np.ascontiguousarray(pr["points"][alive]),
               obs_pt=np.ascontiguousarray(remap[pr["obs_pt"][keep]]))
    for k in ("obs_kf", "obs_uv", "obs_w", "obs_depth"):
        out[k] = np.ascontiguousarray(pr[k][keep])
    return out


def marker_ba_problem(K, P, seed, marker_frames, nfixed=1, het=False, fixed_idx=(1,), extra_frames=0, thin_frame=None, invalid_markers=None,
                      marker_noise=0.003, corner_noise=0.3, **kw):
    """K keyframes in all (extra_frames of them appended without landmarks), P landmarks drawn, marker_frames = one list of keyframes per
    marker.  invalid_markers = {frame: count} adds markers without a valid pose to frame.markers.size().  kw: the keypoint generator's."""
    Kk = K - extra_frames
    kw = dict(QUIET, **kw)
    if het:
        pr = het_ba_synth.het_ba_problem(K=Kk, P=P, seed=seed, fixed_idx=fixed_idx, **kw)
        Tk = het_ba_synth.true_poses(K)
    else:
        pr = stereo_ba_synth.stereo_ba_problem(K=Kk, P=P, seed=seed, nfixed=nfixed, **kw)
        Tk = []
        for k in range(K):
            T = np.eye(4)
            T[:3, 3] = -np.array([0.3 * k, 0.02 * np.sin(k), 0.0])
            Tk.append(synth._se3_exp(np.r_[0.0, 0.02 * np.sin(0.7 * k), 0.0, 0, 0, 0]) @ T)
    rng = np.random.default_rng(30_000 + seed)
    if thin_frame is not None:
        k, n = thin_frame
        mine = np.flatnonzero(pr["obs_kf"] == k)
        drop = np.zeros(pr["E"], bool)
        drop[rng.permutation(mine)[n:]] = True
        pr = _drop_observations(pr, drop)
    if extra_frames:
        pr["poses"] = np.ascontiguousarray(np.concatenate([pr["poses"], np.stack([Tk[k].astype(np.float32).reshape(16) for k in range(Kk, K)])]))
        pr["fixed"] = np.concatenate([pr["fixed"], np.ones(extra_frames, np.uint8)])
        pr["intr"] = np.ascontiguousarray(np.concatenate([pr["intr"], np.tile(pr["intr"][-1], (extra_frames, 1))]))
        pr["frame_bl"] = np.concatenate([pr["frame_bl"], np.tile(pr["frame_bl"][-1:], extra_frames)])
        pr["K"] = K
    I = pr["intr"].astype(np.float64)
    M = len(marker_frames)
    mk_pose = np.zeros((M, 16), np.float32)
    mk_size = np.zeros(M, np.float32)
    em, ef, ec = [], [], []
    for m, frames in enumerate(marker_frames):
        frames = sorted(int(f) for f in frames)
        assert frames and 0 <= frames[0] and frames[-1] < K and len(set(frames)) == len(frames)
        G = np.eye(4)
        # the marker faces the cameras (a half turn about x) with a tilt of up to ~0.4 rad, 2.5-5 m in front of the frames that see it
        G[:3, :3] = _rot(rng.uniform(-0.4, 0.4, 3)) @ _rot(np.array([np.pi, 0, 0]))
        G[:3, 3] = [0.3 * np.mean(frames) + rng.uniform(-0.15, 0.15), rng.uniform(-0.1, 0.1), rng.uniform(2.5, 4.0)]
        G = G.astype(np.float32).astype(np.float64)
        s = np.float32(rng.uniform(0.1, 0.3))
        mk_size[m] = s
        h = float(s) / 2
        C = np.array([[-h, h, 0, 1], [h, h, 0, 1], [h, -h, 0, 1], [-h, -h, 0, 1]])
        for f in frames:
            Pc = (Tk[f] @ G @ C.T).T
            assert (Pc[:, 2] > 0.5).all()
            uv = np.stack([I[f, 0] * Pc[:, 0] / Pc[:, 2] + I[f, 2], I[f, 1] * Pc[:, 1] / Pc[:, 2] + I[f, 3]], 1) + rng.normal(0, corner_noise, (4, 2))
            em.append(m); ef.append(f); ec.append(uv.reshape(8).astype(np.float32))
        mk_pose[m] = (synth._se3_exp(rng.normal(0, np.broadcast_to(marker_noise, M)[m], 6)) @ G).astype(np.float32).reshape(16)
    me_frame = np.array(ef, np.int32)
    n_markers = np.bincount(me_frame, minlength=K).astype(np.int32)
    for f, c in (invalid_markers or {}).items():
        n_markers[f] += c
    weight, kpw = frame_weights(K, pr["obs_kf"], pr["obs_w"], pr["obs_depth"], n_markers)
    pr.update(mk_pose=mk_pose, mk_size=mk_size, me_marker=np.array(em, np.int32), me_frame=me_frame,
              me_corners=np.ascontiguousarray(np.stack(ec)), me_weight=np.ascontiguousarray(weight[me_frame]),
              frame_n_markers=n_markers, frame_kpw=kpw, M=M, EM=len(em))
    return pr


_MULTI = dict(K=6, P=300, extra_frames=1, marker_frames=[[0, 1, 2, 3, 4], [2, 3, 5], [0, 5]])
# mk_hard: the marker that only fixed frames see starts ~1.2 rad / 1.2 m away from where it is, which makes Levenberg-Marquardt reject
# trials (the reject path with the marker chi2 in the sums).  The frames it hangs on do not move, so the keypoint side stays as quiet as
# in the other cases; noise of that size on a marker that free frames see leaves no problem that passes the generator's conditions
# (every rejecting run found ended with most keypoint edges flagged bad and moved by 1e-3 and more under the probes).
HARD = dict(marker_noise=(0.003, 0.003, 1.2))

# the fixture's cases: name -> keyword arguments of marker_ba_problem.  A seed is replaced when tests/golden/make_ba_marker_golden.py
# says that the case does not pass its conditions; FIRST_CHOICE keeps the seeds the cases were first written with.
CASES = {
    "mk_single": dict(K=4, P=120, seed=201, marker_frames=[[0, 1, 2]], stereo_frac=0.0),
    "mk_multi": dict(seed=202, stereo_frac=0.0, **_MULTI),
    "mk_weights": dict(K=5, P=150, seed=203, het=True, fixed_idx=(1,), stereo_frac=0.0, thin_frame=(3, 8), invalid_markers={2: 1},
                       marker_frames=[[0, 1, 3], [2, 3, 4]]),
    "mk_only": dict(K=5, P=0, seed=205, stereo_frac=0.0, marker_frames=[[0, 1], [1, 2], [2, 3], [0, 3, 4]]),
    "mk_stereo": dict(K=6, P=300, seed=205, stereo_frac=0.5, marker_frames=[[0, 1, 2], [3, 4, 5]]),
    "mk_hard": dict(seed=207, stereo_frac=0.0, **_MULTI, **HARD),
    "mk_wide": dict(K=66, P=200, seed=207, stereo_frac=0.0, marker_frames=[[4, 5], [19, 20], [34, 35], [49, 50], [64, 65]]),
}
FIRST_CHOICE = {"mk_single": 201, "mk_multi": 202, "mk_weights": 203, "mk_only": 204, "mk_stereo": 205, "mk_hard": 206, "mk_wide": 207}
