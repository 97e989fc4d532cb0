"""System::relocalize's pose search (src/utils/system.cpp, the statements around raw lines 4950-5500) for the candidate keyframes of ONE
lost frame, composed from the existing mirrors and nothing else:

    set_frame once -> ONE batched uh_pnp_ransac for every candidate with >= 25 matches -> per survivor (>= 15 matches left)
    uh_projmatch_match over that candidate's point list (visible on, radius 2.5) -> the >= 30 gate -> uh_pnp_solve with the look-ups
    uh_track_pose documents (inv_sigma by octave, weight 1 / 0.5) -> the >= 30 gate on good matches -> the candidate with the most
    matches wins, the first on ties.

The candidate selection (uh_bowdb_query) and the descriptor matching (the k-means matcher + uh_match_filter / uh_bowmatch_match) with
the host's list handling stay what they are: the caller passes their outputs in.  The reference ignores solvePnPRansac's return value
and gates on the size of the match list, which a failed call leaves untouched — so does this.
"""
from __future__ import annotations

import numpy as np

from .pnp_ransac import ransac_samples

MIN_MATCHES_RANSAC, MIN_MATCHES_AFTER_RANSAC, MIN_MATCHES_MAP, MIN_GOOD = 25, 15, 30, 30
MAP_RADIUS = 2.5


def se3_to_rt6(pose_f2g) -> np.ndarray:
    """se3::operator=(Mat): the (rvec, tvec) of a 4x4 pose — matrix -> Rodrigues vector in double (the direct axis-angle extraction)."""
    M = np.asarray(pose_f2g, np.float64).reshape(4, 4)
    R = M[:3, :3]
    sk = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = 0.5 * np.linalg.norm(sk), 0.5 * (np.trace(R) - 1)
    th = np.arctan2(s, c)
    rv = 0.5 * sk if s < 1e-5 else sk * (th / (2 * s))
    return np.concatenate([rv, M[:3, 3]]).astype(np.float32)


def relocalize_pose(pm, pnp, ransac, frame, candidates, inv_sigma_levels, max_desc_dist, max_iters=50):
    """pm / pnp / ransac: ProjectionMatcher, PnPSolver, PnPRansac on one context.
    frame: dict(und_kpts (KEYPOINT_DTYPE), desc, scale_factors, fx, fy, cx, cy, min_xy, max_xy) as ProjectionMatcher.setFrame takes it.
    candidates: one dict per candidate keyframe, in the order of Map::relocalizationCandidates:
        matches   DMATCH_DTYPE, queryIdx = the frame's keypoint, trainIdx = the map point's id (after the host's list handling)
        p3d, normal   (len(matches), 3): that map point's coordinates and normal
        rt6       the keyframe's pose_f2g as (rvec, tvec)
        points    dict(ids, pos3d, normal, min_dist, max_dist, desc, weight): the points of getNeighborsVLevel2(kf, true)
        samples   optional (max_iters, 4): else drawn from libc rand() as the reference draws them, candidate by candidate
    max_desc_dist: System's maxDescDistance (the projection search runs with twice that).
    Returns dict(best = index of the winning candidate or -1, pose (4, 4) or None, n_matches, steps = per candidate dict(stage, ransac,
    matches_ransac, pose_ransac, matches_map, solve, matches_final))."""
    pm.setFrame(frame["und_kpts"], frame["desc"], frame["scale_factors"], frame["fx"], frame["fy"], frame["cx"], frame["cy"],
                frame.get("min_xy", (0, 0)), frame.get("max_xy", (2 ** 31 - 1, 2 ** 31 - 1)))
    kps = frame["und_kpts"]
    intr4 = np.array([frame["fx"], frame["fy"], frame["cx"], frame["cy"]], np.float32)
    isl = np.ascontiguousarray(inv_sigma_levels, np.float32)
    steps = [dict(stage="matches < 25") for _ in candidates]
    live, problems = [], []
    for c, cand in enumerate(candidates):
        m = cand["matches"]
        if len(m) < MIN_MATCHES_RANSAC:
            continue
        q = m["queryIdx"]
        smp = cand.get("samples")
        if smp is None:
            smp = ransac_samples(len(m), max_iters)
        live.append(c)
        problems.append(dict(p3d=cand["p3d"], normal=cand["normal"], kp=np.stack([kps["x"][q], kps["y"][q]], 1), samples=smp, rt6_in=cand["rt6"]))
    results = ransac.solve(intr4, problems) if problems else []
    best, best_n, best_pose = -1, 0, None
    for c, r in zip(live, results):
        cand, st = candidates[c], steps[c]
        m = cand["matches"][r["inliers"]] if r["ok"] else cand["matches"]
        st.update(ransac=r, matches_ransac=m, pose_ransac=r["pose"], stage="matches < 15 after RANSAC")
        if len(m) < MIN_MATCHES_AFTER_RANSAC:
            continue
        pts = cand["points"]
        b = pm.matchFrameToMapPoints(r["pose"], pts["ids"], pts["pos3d"], pts["normal"], pts["min_dist"], pts["max_dist"], pts["desc"], 2 * max_desc_dist, MAP_RADIUS)
        m = b["matches"]
        st.update(matches_map=m, stage="matches < 30 after the projection search")
        if len(m) < MIN_MATCHES_MAP:
            continue
        row = {int(v): i for i, v in enumerate(np.asarray(pts["ids"]))}
        rows = np.array([row[int(t)] for t in m["trainIdx"]], np.int64)
        q = m["queryIdx"]
        s = pnp.solvePnp(r["pose"], intr4, np.asarray(pts["pos3d"], np.float32)[rows], np.stack([kps["x"][q], kps["y"][q]], 1), isl[kps["octave"][q]],
                         np.asarray(pts["weight"], np.float32)[rows])
        good = m[s["bad"][: len(m)] == 0]
        st.update(solve=s, matches_final=good, stage="good matches < 30")
        if len(good) < MIN_GOOD:
            continue
        st["stage"] = "solved"
        if len(good) > best_n:
            best, best_n, best_pose = c, len(good), s["pose"].reshape(4, 4).copy()
    return dict(best=best, pose=best_pose, n_matches=best_n, steps=steps)
