"""relocalize_pose (ucoslam-cv3_amd/relocalize.py): System::relocalize's pose search for the candidates of one lost frame, composed from
uh_pnp_ransac, uh_projmatch_match and uh_pnp_solve.  A synthetic map and one frame (tests/synth.py, as the projection-matcher and
tracker tests use them), three candidates: the true neighbourhood, one with 20 matches (stopped at the first gate) and one whose
40 matches are wrong but for eight (a keyframe that shares a handful of points by chance: RANSAC succeeds on those eight, the list shrinks to
fewer than 15 and the candidate is stopped right after RANSAC).  The true candidate wins, its pose is
within the PnP tests' tolerance of the planted pose, and every intermediate list equals what the operators give one by one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu
MAX_DESC_DIST = 50.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_relocalize_example_runs(tmp_path):
    """examples/relocalize.cpp: the same chain from a C++ host over the C ABI, on its own synthetic inputs."""
    lib_dir = os.path.join(ROOT, "ucoslam-cv3_amd")
    exe = str(tmp_path / "relocalize")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", exe, os.path.join(ROOT, "examples", "relocalize.cpp"), "-L", lib_dir, "-lucoslam_hip",
                           f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "relocalised on candidate 0" in out.stdout and "candidate 1: 20 matches, below 25" in out.stdout, out.stdout + out.stderr


def test_relocalize_pose_picks_the_true_candidate(hip_ctx):
    from ucoslam_cv3_amd import PnPRansac, ransac_samples
    from ucoslam_cv3_amd.pnp import PnPSolver
    from ucoslam_cv3_amd.projmatch import ProjectionMatcher
    from ucoslam_cv3_amd.relocalize import relocalize_pose, se3_to_rt6

    fr, mp, pose_kf = synth.proj_problem(2000, 3000, seed=31)
    planted = synth._se3_exp(np.r_[0.01, -0.015, 0.004, 0, 0, 0])
    planted[:3, 3] = [0.3, -0.05, 0.1]
    rng = np.random.default_rng(5)
    mp = dict(mp, weight=np.where(rng.random(len(mp["ids"])) < 0.2, np.float32(0.5), np.float32(1)).astype(np.float32))
    pm, pnp = ProjectionMatcher(hip_ctx), PnPSolver(hip_ctx)
    ransac = PnPRansac(pnp)
    sf = fr["scale_factors"]
    inv_sf = (np.float32(1) / sf).astype(np.float32)
    intr = np.array([fr["fx"], fr["fy"], fr["cx"], fr["cy"]], np.float32)
    # the descriptor matcher's part, played by a wide projection search from the keyframe's (nearby) pose: keypoint <-> map point id
    pm.setFrame(fr["und_kpts"], fr["desc"], sf, fr["fx"], fr["fy"], fr["cx"], fr["cy"], fr["min_xy"], fr["max_xy"])
    m0 = pm.matchFrameToMapPoints(pose_kf, mp["ids"], mp["pos3d"], mp["normal"], mp["min_dist"], mp["max_dist"], mp["desc"], 2 * MAX_DESC_DIST, 15.0)["matches"]
    assert len(m0) > 200
    row = {int(v): i for i, v in enumerate(mp["ids"])}
    rows = np.array([row[int(t)] for t in m0["trainIdx"]], np.int64)
    rt6 = se3_to_rt6(pose_kf)
    C.CDLL(None).srand(C.c_uint(99))
    true_c = dict(matches=m0, p3d=mp["pos3d"][rows], normal=mp["normal"][rows], rt6=rt6, points=mp, samples=ransac_samples(len(m0), 50))
    few_c = dict(matches=m0[:20], p3d=mp["pos3d"][rows[:20]], normal=mp["normal"][rows[:20]], rt6=rt6, points=mp)
    # the wrong candidate: eight matches that fit the planted pose to a pixel, 32 keypoints paired with another point's coordinates; its first
    # sample is four of the eight, so one hypothesis is sure to find them
    q0 = m0["queryIdx"]
    Xc = mp["pos3d"][rows].astype(np.float64) @ planted[:3, :3].T + planted[:3, 3]
    err = np.hypot(fr["fx"] * Xc[:, 0] / Xc[:, 2] + fr["cx"] - fr["und_kpts"]["x"][q0], fr["fy"] * Xc[:, 1] / Xc[:, 2] + fr["cy"] - fr["und_kpts"]["y"][q0])
    fit = np.nonzero(err < 1.0)[0]
    good8 = fit[np.linspace(0, len(fit) - 1, 8).astype(np.int64)]
    bad32 = np.setdiff1d(np.arange(len(m0)), good8)[:32]
    sel = np.concatenate([good8, bad32])
    p3d_w, nrm_w = mp["pos3d"][rows][sel].copy(), mp["normal"][rows][sel].copy()
    p3d_w[8:], nrm_w[8:] = np.roll(p3d_w[8:], 5, axis=0), np.roll(nrm_w[8:], 5, axis=0)
    smp_w = ransac_samples(40, 50)
    smp_w[0] = [0, 3, 5, 7]
    wrong_c = dict(matches=m0[sel], p3d=p3d_w, normal=nrm_w, rt6=rt6, points=mp, samples=smp_w)
    cands = [few_c, wrong_c, true_c]
    out = relocalize_pose(pm, pnp, ransac, fr, cands, inv_sf, MAX_DESC_DIST)
    st = out["steps"]
    print("stages:", [s["stage"] for s in st], "matches", out["n_matches"])
    assert out["best"] == 2 and st[2]["stage"] == "solved" and out["n_matches"] >= 30
    assert st[0]["stage"] == "matches < 25" and "ransac" not in st[0]
    # the wrong candidate is stopped after RANSAC: it succeeds on the handful of right matches, and fewer than 15 are left
    assert st[1]["ransac"]["ok"] == 1 and 4 <= st[1]["ransac"]["n_inliers"] < 15 and set(st[1]["ransac"]["inliers"].tolist()) <= set(range(8))
    assert st[1]["stage"] == "matches < 15 after RANSAC" and "matches_map" not in st[1]
    # the PnP tests' bar against a planted pose (tests/test_pnp.py): translation within 0.01
    print("translation error", np.abs(out["pose"][:3, 3] - planted[:3, 3]).max(), "rotation", np.abs(out["pose"][:3, :3] - planted[:3, :3]).max())
    assert np.abs(out["pose"][:3, 3] - planted[:3, 3]).max() < 0.01

    # ---- the same through the operators one by one
    kps = fr["und_kpts"]
    for c in (1, 2):
        cand = cands[c]
        q = cand["matches"]["queryIdx"]
        r = ransac.solve(intr, [dict(p3d=cand["p3d"], normal=cand["normal"], kp=np.stack([kps["x"][q], kps["y"][q]], 1), samples=cand["samples"], rt6_in=rt6)])[0]
        g = st[c]["ransac"]
        assert (r["ok"], r["best_iter"]) == (g["ok"], g["best_iter"]) and np.array_equal(r["inliers"], g["inliers"]) and r["pose"].tobytes() == g["pose"].tobytes()
        want = cand["matches"][r["inliers"]] if r["ok"] else cand["matches"]
        assert st[c]["matches_ransac"].tobytes() == want.tobytes()
        if "matches_map" not in st[c]:
            assert len(want) < 15
            continue
        b = pm.matchFrameToMapPoints(r["pose"], mp["ids"], mp["pos3d"], mp["normal"], mp["min_dist"], mp["max_dist"], mp["desc"], 2 * MAX_DESC_DIST, 2.5)
        assert st[c]["matches_map"].tobytes() == b["matches"].tobytes()
    m = st[2]["matches_map"]
    rows2 = np.array([row[int(t)] for t in m["trainIdx"]], np.int64)
    q = m["queryIdx"]
    s = pnp.solvePnp(st[2]["pose_ransac"], intr, mp["pos3d"][rows2], np.stack([kps["x"][q], kps["y"][q]], 1), inv_sf[kps["octave"][q]], mp["weight"][rows2])
    assert s["pose"].tobytes() == st[2]["solve"]["pose"].tobytes() and np.array_equal(s["bad"], st[2]["solve"]["bad"]) and s["ngood"] == st[2]["solve"]["ngood"]
    assert st[2]["matches_final"].tobytes() == m[s["bad"][: len(m)] == 0].tobytes() and np.array_equal(out["pose"].reshape(16), s["pose"])
