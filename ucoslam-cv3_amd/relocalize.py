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

import ctypes as C

import numpy as np

from . import _lib
from ._lib import I, VP, check, lib, np_ptr
from .pnp_ransac import ransac_samples
from .projmatch import DMATCH_DTYPE, _MapPoints

MIN_MATCHES_RANSAC, MIN_MATCHES_AFTER_RANSAC, MIN_MATCHES_MAP, MIN_GOOD = 25, 15, 30, 30
MAP_RADIUS = 2.5
STAGES = ("matches < 25", "matches < 15 after RANSAC", "matches < 30 after the projection search", "good matches < 30", "solved")   # UH_RELOC_* 0..4


class _RelocArgs(C.Structure):   # uh_reloc_args
    _fields_ = [("intr4", VP), ("inv_sigma_levels", VP), ("n_levels", C.c_int32), ("map_min_desc_dist", C.c_float), ("map_radius", C.c_float),
                ("max_iters", C.c_int32), ("min_matches_ransac", C.c_int32), ("min_matches_after_ransac", C.c_int32), ("min_matches_map", C.c_int32),
                ("min_good", C.c_int32)]


class _RelocCandidate(C.Structure):   # uh_reloc_candidate
    _fields_ = [("n", C.c_int32), ("query_idx", VP), ("p3d", VP), ("normal", VP), ("rt6_in", VP), ("samples", VP), ("points", C.POINTER(_MapPoints)),
                ("weight", VP)]


class _RelocStep(C.Structure):   # uh_reloc_step
    _fields_ = [("stage", C.c_int32), ("ok", C.c_int32), ("n_inliers", C.c_int32), ("best_iter", C.c_int32), ("rt6", C.c_float * 6),
                ("pose_ransac", C.c_float * 16), ("inliers", VP), ("cap_inliers", C.c_int32), ("n_map", C.c_int32), ("matches_map", VP), ("bad", VP),
                ("cap_map", C.c_int32), ("pose_solve", C.c_float * 16), ("iters", C.c_int32 * 4), ("solve_inliers", C.c_int32), ("n_good", C.c_int32)]


class _RelocResult(C.Structure):   # uh_reloc_result
    _fields_ = [("best", C.c_int32), ("pose", C.c_float * 16), ("n_matches", C.c_int32), ("steps", C.POINTER(_RelocStep))]


def _declare(L, sig):
    sig("uh_relocalize_pose", I, VP, VP, C.POINTER(_RelocArgs), I, C.POINTER(_RelocCandidate), C.POINTER(_RelocResult))


_lib._EXTRA_DECLS.append(_declare)


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


def relocalize_pose_onecall(pm, pnp, ransac, frame, candidates, inv_sigma_levels, max_desc_dist, max_iters=50, gates=None, n_keypoints=None):
    """relocalize_pose as ONE call (uh_relocalize_pose, csrc/relocalize.hpp): the same arguments, the same dict, bit for bit — but the
    matcher's frame must already be the device-resident one (ProjectionMatcher.setFrameDev over a DeviceFrame that was extracted or
    uploaded): `frame` only gives the intrinsics here, and `ransac` is unused (the solver object of `pnp` serves).  A candidate's
    `matches` give queryIdx; trainIdx of matches_map comes from the call.  candidates without `samples` have them drawn inside the call.
    gates: (min_matches_ransac, min_matches_after_ransac, min_matches_map, min_good), default (25, 15, 30, 30).  n_keypoints: the frame's
    keypoint count (sizes the result buffers; default 4096, the call's limit).
    steps[c]["ransac"] has no per-hypothesis `counts` (None); steps[c]["solve"] holds pose, bad, iters, ngood (the solver's inlier count)."""
    g = tuple(gates) if gates is not None else (MIN_MATCHES_RANSAC, MIN_MATCHES_AFTER_RANSAC, MIN_MATCHES_MAP, MIN_GOOD)
    nk = 4096 if n_keypoints is None else int(n_keypoints)
    intr4 = np.array([frame["fx"], frame["fy"], frame["cx"], frame["cy"]], np.float32)
    isl = np.ascontiguousarray(inv_sigma_levels, np.float32)
    args = _RelocArgs(np_ptr(intr4), np_ptr(isl), len(isl), float(2 * max_desc_dist), float(MAP_RADIUS), int(max_iters), *[int(v) for v in g])
    m = len(candidates)
    cs, ss = (_RelocCandidate * max(m, 1))(), (_RelocStep * max(m, 1))()
    keep, bufs = [], []

    def arr(x, dt, shape=None):
        a = np.ascontiguousarray(x, dt)
        a = a.reshape(shape) if shape is not None else a
        keep.append(a)
        return a

    for c, cand in enumerate(candidates):
        mt = cand["matches"]
        n = len(mt)
        q = arr(mt["queryIdx"], np.int32)
        p3d, nrm, rt6 = arr(cand["p3d"], np.float32, (-1, 3)), arr(cand["normal"], np.float32, (-1, 3)), arr(cand["rt6"], np.float32, 6)
        smp = arr(cand["samples"], np.int32, (-1, 4)) if cand.get("samples") is not None else None
        pts = cand["points"]
        ids = arr(pts["ids"], np.uint32)
        npt = len(ids)
        pa = [arr(pts["pos3d"], np.float32, (npt, 3)), arr(pts["normal"], np.float32, (npt, 3)), arr(pts["min_dist"], np.float32), arr(pts["max_dist"], np.float32),
              arr(pts["desc"], np.uint8, (npt, 32))]
        mpp = _MapPoints(npt, np_ptr(ids) if npt else None, *[np_ptr(x) if npt else None for x in pa])
        keep.append(mpp)
        w = arr(pts["weight"], np.float32) if pts.get("weight") is not None else None
        cs[c] = _RelocCandidate(n, np_ptr(q) if n else None, np_ptr(p3d) if n else None, np_ptr(nrm) if n else None, np_ptr(rt6),
                                np_ptr(smp) if smp is not None else None, C.pointer(mpp), np_ptr(w) if w is not None and npt else None)
        cap = max(min(npt, nk), 1)
        inl, mm, bad = np.zeros(max(n, 1), np.int32), np.zeros(cap, DMATCH_DTYPE), np.zeros(cap, np.uint8)
        bufs.append((inl, mm, bad))
        ss[c].inliers, ss[c].cap_inliers, ss[c].matches_map, ss[c].bad, ss[c].cap_map = np_ptr(inl), len(inl), np_ptr(mm), np_ptr(bad), cap
    res = _RelocResult()
    res.steps = C.cast(ss, C.POINTER(_RelocStep))
    check(lib().uh_relocalize_pose(pm._h, pnp._h, C.byref(args), m, C.cast(cs, C.POINTER(_RelocCandidate)), C.byref(res)))
    steps = []
    for c, cand in enumerate(candidates):
        s, (inl, mm, bad) = ss[c], bufs[c]
        st = dict(stage=STAGES[s.stage])
        if s.stage >= 1:
            r = dict(ok=int(s.ok), n_inliers=int(s.n_inliers), best_iter=int(s.best_iter), rt6=np.array(s.rt6[:], np.float32),
                     pose=np.array(s.pose_ransac[:], np.float32).reshape(4, 4), inliers=inl[: s.n_inliers].copy(), counts=None)
            st.update(ransac=r, matches_ransac=cand["matches"][r["inliers"]] if r["ok"] else cand["matches"], pose_ransac=r["pose"])
        if s.stage >= 2:
            st.update(matches_map=mm[: s.n_map].copy())
        if s.stage >= 3:
            sv = dict(pose=np.array(s.pose_solve[:], np.float32), bad=bad[: s.n_map].copy(), iters=np.array(s.iters[:], np.int32), ngood=int(s.solve_inliers))
            st.update(solve=sv, matches_final=st["matches_map"][bad[: s.n_map] == 0])
        steps.append(st)
    best = int(res.best)
    return dict(best=best, pose=np.array(res.pose[:], np.float32).reshape(4, 4) if best >= 0 else None, n_matches=int(res.n_matches), steps=steps)
