"""uh_relocalize_pose (csrc/relocalize.hpp) — System::relocalize's pose search for all candidates of one lost frame as ONE call — against
the composed chain relocalize_pose (uh_pnp_ransac -> per survivor uh_projmatch_match -> look-ups -> uh_pnp_solve): every stage, RANSAC
field, list, flag, count and pose byte for byte, no tolerance.  The composed chain runs on a matcher with the host-side frame, the one
call on a second matcher whose frame is the same keypoints and descriptors uploaded as a device-resident frame.

The gates: 24 / 25 matches are made by trimming the match list.  The counts behind RANSAC, behind the projection search and n_good come
out of the operators, so those gates are tested by passing the gate itself (they are arguments of the call) at the count the composed
chain shows and one above it: the candidate passes at the first and is stopped at the second."""
import ctypes as C

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu
MAX_DESC_DIST = 50.0
GATES = (25, 15, 30, 30)


class _Scene:
    def __init__(self, hip_ctx, n_kpts=2000, n_pts=3000, seed=31):
        from ucoslam_cv3_amd import PnPRansac, ransac_samples
        from ucoslam_cv3_amd.orb import DeviceFrame
        from ucoslam_cv3_amd.pnp import PnPSolver
        from ucoslam_cv3_amd.projmatch import ProjectionMatcher
        from ucoslam_cv3_amd.relocalize import se3_to_rt6

        self.ctx = hip_ctx
        fr, mp, pose_kf = synth.proj_problem(n_kpts, n_pts, seed=seed)
        rng = np.random.default_rng(5)
        self.fr, self.pose_kf = fr, pose_kf
        self.mp = dict(mp, weight=np.where(rng.random(len(mp["ids"])) < 0.2, np.float32(0.5), np.float32(1)).astype(np.float32))
        self.sf = fr["scale_factors"]
        self.inv_sf = (np.float32(1) / self.sf).astype(np.float32)
        self.planted = synth._se3_exp(np.r_[0.01, -0.015, 0.004, 0, 0, 0])
        self.planted[:3, 3] = [0.3, -0.05, 0.1]
        self.pm_host, self.pnp_host = ProjectionMatcher(hip_ctx), PnPSolver(hip_ctx)
        self.ransac = PnPRansac(self.pnp_host)
        self.pm, self.pnp = self.fresh()
        mp = self.mp
        pmh = self.pm_host
        pmh.setFrame(fr["und_kpts"], fr["desc"], self.sf, fr["fx"], fr["fy"], fr["cx"], fr["cy"], fr["min_xy"], fr["max_xy"])
        # the descriptor matcher's part, played by a wide projection search from the keyframe's (nearby) pose (as tests/test_relocalize.py)
        m0 = pmh.matchFrameToMapPoints(pose_kf, mp["ids"], mp["pos3d"], mp["normal"], mp["min_dist"], mp["max_dist"], mp["desc"], 2 * MAX_DESC_DIST, 15.0)["matches"]
        assert len(m0) > 200
        row = {int(v): i for i, v in enumerate(mp["ids"])}
        self.m0, self.rows = m0, np.array([row[int(t)] for t in m0["trainIdx"]], np.int64)
        self.rt6 = se3_to_rt6(pose_kf)
        C.CDLL(None).srand(C.c_uint(99))
        self.smp_true = ransac_samples(len(m0), 50)
        self.smp_40 = ransac_samples(40, 50)

    def fresh(self):
        """A matcher with the frame uploaded as a device-resident one, and a solver: the objects of the one call."""
        from ucoslam_cv3_amd.orb import DeviceFrame
        from ucoslam_cv3_amd.pnp import PnPSolver
        from ucoslam_cv3_amd.projmatch import ProjectionMatcher

        fr = self.fr
        dev = DeviceFrame(self.ctx).upload(fr["und_kpts"], fr["desc"])
        pm = ProjectionMatcher(self.ctx)
        pm.setFrameDev(dev, self.sf, fr["fx"], fr["fy"], fr["cx"], fr["cy"], fr["min_xy"], fr["max_xy"], und_kpts=fr["und_kpts"])
        return pm, PnPSolver(self.ctx)

    # ---- candidates
    def true_c(self, n=None, samples=True, points=None):
        from ucoslam_cv3_amd import ransac_samples

        n = len(self.m0) if n is None else n
        c = dict(matches=self.m0[:n], p3d=self.mp["pos3d"][self.rows[:n]], normal=self.mp["normal"][self.rows[:n]], rt6=self.rt6, points=self.mp if points is None else points)
        if samples and n >= 4:
            c["samples"] = self.smp_true if n == len(self.m0) else ransac_samples(n, 50)
        return c

    def wrong_c(self, n_good=8, n_bad=32, first=(0, 3, 5, 7), samples=True):
        """n_good matches that fit the planted pose to a pixel, n_bad keypoints paired with another point's coordinates."""
        fr, mp, rows, m0 = self.fr, self.mp, self.rows, self.m0
        q0 = m0["queryIdx"]
        Xc = mp["pos3d"][rows].astype(np.float64) @ self.planted[:3, :3].T + self.planted[:3, 3]
        err = np.hypot(fr["fx"] * Xc[:, 0] / Xc[:, 2] + fr["cx"] - fr["und_kpts"]["x"][q0], fr["fy"] * Xc[:, 1] / Xc[:, 2] + fr["cy"] - fr["und_kpts"]["y"][q0])
        fit = np.nonzero(err < 1.0)[0]
        good = fit[np.linspace(0, len(fit) - 1, n_good).astype(np.int64)] if n_good else np.zeros(0, np.int64)
        bad = np.setdiff1d(np.arange(len(m0)), good)[:n_bad]
        sel = np.concatenate([good, bad])
        p3d_w, nrm_w = mp["pos3d"][rows][sel].copy(), mp["normal"][rows][sel].copy()
        p3d_w[n_good:], nrm_w[n_good:] = np.roll(p3d_w[n_good:], 5, axis=0), np.roll(nrm_w[n_good:], 5, axis=0)
        c = dict(matches=m0[sel], p3d=p3d_w, normal=nrm_w, rt6=self.rt6, points=mp)
        if samples:
            smp = self.smp_40.copy() if len(sel) == 40 else __import__("ucoslam_cv3_amd").ransac_samples(len(sel), 50)
            if first is not None:
                smp[0] = first
            c["samples"] = smp
        return c

    def sub_points(self, keep):
        return {k: np.ascontiguousarray(v[keep]) for k, v in self.mp.items()}

    # ---- the two routes
    def composed(self, cands, gates=GATES):
        from ucoslam_cv3_amd import relocalize as R

        old = (R.MIN_MATCHES_RANSAC, R.MIN_MATCHES_AFTER_RANSAC, R.MIN_MATCHES_MAP, R.MIN_GOOD)
        R.MIN_MATCHES_RANSAC, R.MIN_MATCHES_AFTER_RANSAC, R.MIN_MATCHES_MAP, R.MIN_GOOD = gates
        try:
            return R.relocalize_pose(self.pm_host, self.pnp_host, self.ransac, self.fr, cands, self.inv_sf, MAX_DESC_DIST)
        finally:
            R.MIN_MATCHES_RANSAC, R.MIN_MATCHES_AFTER_RANSAC, R.MIN_MATCHES_MAP, R.MIN_GOOD = old

    def onecall(self, cands, gates=GATES, objs=None, **kw):
        from ucoslam_cv3_amd.relocalize import relocalize_pose_onecall

        pm, pnp = objs if objs is not None else (self.pm, self.pnp)
        return relocalize_pose_onecall(pm, pnp, None, self.fr, cands, self.inv_sf, MAX_DESC_DIST, gates=gates, n_keypoints=len(self.fr["und_kpts"]), **kw)


@pytest.fixture(scope="module")
def sc(hip_ctx):
    return _Scene(hip_ctx)


def _same_step(a, b, where):
    assert a["stage"] == b["stage"], (where, a["stage"], b["stage"])
    assert set(a) == set(b), (where, sorted(a), sorted(b))
    if "ransac" in a:
        ra, rb = a["ransac"], b["ransac"]
        assert (ra["ok"], ra["n_inliers"], ra["best_iter"]) == (rb["ok"], rb["n_inliers"], rb["best_iter"]), where
        assert ra["rt6"].tobytes() == rb["rt6"].tobytes() and ra["pose"].tobytes() == rb["pose"].tobytes(), where
        assert np.array_equal(ra["inliers"], rb["inliers"]), where
        assert a["matches_ransac"].tobytes() == b["matches_ransac"].tobytes() and a["pose_ransac"].tobytes() == b["pose_ransac"].tobytes(), where
    if "matches_map" in a:
        assert a["matches_map"].tobytes() == b["matches_map"].tobytes(), (where, len(a["matches_map"]), len(b["matches_map"]))
    if "solve" in a:
        sa, sb = a["solve"], b["solve"]
        assert sa["pose"].tobytes() == sb["pose"].tobytes() and np.array_equal(sa["bad"], sb["bad"]) and np.array_equal(sa["iters"], sb["iters"]), where
        assert sa["ngood"] == sb["ngood"] and a["matches_final"].tobytes() == b["matches_final"].tobytes(), where


def _same(a, b):
    assert a["best"] == b["best"] and a["n_matches"] == b["n_matches"], (a["best"], b["best"], a["n_matches"], b["n_matches"])
    assert (a["pose"] is None) == (b["pose"] is None)
    if a["pose"] is not None:
        assert np.asarray(a["pose"], np.float32).tobytes() == np.asarray(b["pose"], np.float32).tobytes()
    assert len(a["steps"]) == len(b["steps"])
    for c, (x, y) in enumerate(zip(a["steps"], b["steps"])):
        _same_step(x, y, "candidate %d" % c)


def test_three_candidates(sc):
    cands = [sc.true_c(20), sc.wrong_c(), sc.true_c()]
    want, got = sc.composed(cands), sc.onecall(cands)
    assert want["best"] == 2 and [s["stage"] for s in want["steps"]] == ["matches < 25", "matches < 15 after RANSAC", "solved"]
    _same(want, got)
    assert got["best"] == 2


def test_gate_on_the_match_count(sc):
    cands = [sc.true_c(24), sc.true_c(25)]
    want = sc.composed(cands)
    assert want["steps"][0]["stage"] == "matches < 25" and "ransac" in want["steps"][1] and len(cands[0]["matches"]) == 24 and len(cands[1]["matches"]) == 25
    _same(want, sc.onecall(cands))


def _count(step, gate):
    if gate == 1:
        return len(step["matches_ransac"])
    return len(step["matches_map"]) if gate == 2 else len(step["matches_final"])


@pytest.mark.parametrize("gate", [1, 2, 3])
def test_gates_on_both_sides(sc, gate):
    """gate 1: the count after RANSAC (a candidate whose RANSAC keeps a handful of inliers), 2: the projection search's matches (the true
    candidate over a part of its points), 3: n_good (the same).  The gate is put at the observed count (passes) and one above (stopped)."""
    cand = sc.wrong_c(n_good=16, n_bad=24) if gate == 1 else sc.true_c(points=sc.sub_points(np.arange(0, len(sc.mp["ids"]), 12)))
    loose = [25, 1, 1, 1]
    base = sc.composed([cand], tuple(loose))["steps"][0]
    n = _count(base, gate)
    print("gate", gate, "observed count", n, "stage", base["stage"])
    assert n >= 1
    stopped = ("matches < 15 after RANSAC", "matches < 30 after the projection search", "good matches < 30")[gate - 1]
    for g, passes in ((n, True), (n + 1, False)):
        gates = list(loose)
        gates[gate] = g
        want = sc.composed([cand], tuple(gates))
        assert _count(want["steps"][0], gate) == n and (want["steps"][0]["stage"] != stopped) == passes, (g, want["steps"][0]["stage"])
        _same(want, sc.onecall([cand], tuple(gates)))


def test_failed_ransac_goes_on(sc):
    """ok == 0 with a winner (its pose is kept, every match stays) and no winner at all (collinear points: every sample is skipped, the pose
    is Se3Transform(rt6_in)); both reach the projection search."""
    from ucoslam_cv3_amd import ransac_samples

    fail = None
    for k in range(12):   # all matches wrong: the best hypothesis explains its own sample at most
        c = sc.wrong_c(n_good=0, n_bad=30 + k, first=None)
        s = sc.composed([c])["steps"][0]
        if s["ransac"]["ok"] == 0 and s["ransac"]["best_iter"] >= 0:
            fail = c
            break
    assert fail is not None
    n = 40
    t = np.linspace(-1, 1, n)[:, None]
    line = (np.array([[0.5, 0.2, 12.0]]) + t * np.array([[1.0, 0.3, 0.5]])).astype(np.float32)
    col = dict(matches=sc.m0[:n], p3d=line, normal=sc.mp["normal"][sc.rows[:n]], rt6=sc.rt6, points=sc.mp, samples=ransac_samples(n, 50))
    cands = [fail, col]
    want = sc.composed(cands)
    s0, s1 = want["steps"]
    assert s0["ransac"]["ok"] == 0 and s0["ransac"]["best_iter"] >= 0 and len(s0["matches_ransac"]) == len(fail["matches"]) and "matches_map" in s0
    assert s1["ransac"]["ok"] == 0 and s1["ransac"]["best_iter"] == -1 and np.array_equal(s1["ransac"]["rt6"], sc.rt6) and "matches_map" in s1
    _same(want, sc.onecall(cands))


def test_ties(sc):
    weak = sc.true_c(points=sc.sub_points(np.arange(0, len(sc.mp["ids"]), 3)))
    for cands, best in (([sc.true_c(), sc.true_c()], 0), ([weak, sc.true_c(), sc.true_c()], 1)):
        want = sc.composed(cands)
        assert want["best"] == best and all(s["stage"] == "solved" for s in want["steps"])
        assert want["steps"][-1]["solve"]["ngood"] == want["steps"][-2]["solve"]["ngood"]
        _same(want, sc.onecall(cands))


def test_no_survivor_and_the_empty_call(sc):
    empty_pts = sc.sub_points(np.zeros(0, np.int64))
    none_c = dict(matches=sc.m0[:0], p3d=np.zeros((0, 3), np.float32), normal=np.zeros((0, 3), np.float32), rt6=sc.rt6, points=sc.mp)
    few_pts = sc.true_c(points=sc.sub_points(np.arange(0, len(sc.mp["ids"]), 60)))
    cands = [sc.true_c(20), sc.wrong_c(), sc.true_c(points=empty_pts), none_c, few_pts]
    want = sc.composed(cands)
    assert want["best"] == -1 and want["pose"] is None
    assert [s["stage"] for s in want["steps"]][:4] == ["matches < 25", "matches < 15 after RANSAC", "matches < 30 after the projection search", "matches < 25"]
    _same(want, sc.onecall(cands))
    got = sc.onecall([])
    assert got["best"] == -1 and got["pose"] is None and got["n_matches"] == 0 and got["steps"] == []
    _same(sc.composed([]), got)


def test_samples_drawn_by_the_call(sc):
    libc = C.CDLL(None)
    cands = [sc.true_c(samples=False), sc.true_c(20, samples=False), sc.wrong_c(samples=False)]
    libc.srand(C.c_uint(1234))
    want = sc.composed(cands)
    r_want = libc.rand()
    libc.srand(C.c_uint(1234))
    got = sc.onecall(cands)
    r_got = libc.rand()
    assert r_want == r_got
    _same(want, got)
    assert want["best"] == 0


def _eight(sc):
    n = len(sc.mp["ids"])
    return [sc.true_c(), sc.wrong_c(), sc.true_c(20), sc.true_c(points=sc.sub_points(np.arange(0, n, 3))), sc.true_c(120), sc.wrong_c(n_good=16, n_bad=24),
            sc.true_c(points=sc.sub_points(np.arange(1, n, 2))), sc.true_c(60, points=sc.sub_points(np.arange(0, n, 40)))]


def test_batch_independence(sc):
    cands = _eight(sc)
    objs = sc.fresh()
    all8 = sc.onecall(cands, objs=objs)
    _same(sc.composed(cands), all8)
    for c, cand in enumerate(cands):
        _same_step(all8["steps"][c], sc.onecall([cand], objs=sc.fresh())["steps"][0], "candidate %d alone" % c)
    three = [cands[6], cands[2], cands[3]]
    _same(sc.onecall(three, objs=sc.fresh()), sc.onecall(three, objs=objs))   # (after the call of eight on the same objects)
    _same(sc.composed(three), sc.onecall(three, objs=objs))


def test_coexists_with_the_tracker(sc):
    pm, pnp = sc.fresh()
    mp, kps = sc.mp, sc.fr["und_kpts"]
    prev = dict(ids=mp["ids"][sc.rows], pos3d=mp["pos3d"][sc.rows], octave=kps["octave"][sc.m0["queryIdx"]].astype(np.int32), desc=mp["desc"][sc.rows])
    intr = np.array([sc.fr["fx"], sc.fr["fy"], sc.fr["cx"], sc.fr["cy"]], np.float32)

    def track():
        return pm.trackPose(pnp, sc.pose_kf, intr, sc.inv_sf, prev, mp, prev_map_row=sc.rows.astype(np.int32), map_weight=mp["weight"])

    t1 = track()
    cands = [sc.true_c(), sc.wrong_c()]
    _same(sc.composed(cands), sc.onecall(cands, objs=(pm, pnp)))
    t2 = track()
    assert len(t1["matches_prev"]) > 30
    for k in t1:
        assert np.asarray(t1[k]).tobytes() == np.asarray(t2[k]).tobytes(), k


def test_more_matches_than_the_solver_keeps_in_lds(hip_ctx):
    """One frame of 4096 keypoints and a point list that gives more than kPnpLdsMatches (3000) matches, beside a small candidate."""
    big = _Scene(hip_ctx, 4096, 30000, seed=7)
    cands = [big.true_c(), big.true_c(200, points=big.sub_points(np.arange(0, 30000, 20)))]
    want = big.composed(cands)
    print("matches of the projection search:", [len(s.get("matches_map", [])) for s in want["steps"]])
    assert len(want["steps"][0]["matches_map"]) > 3000
    _same(want, big.onecall(cands))


def test_refusals(sc):
    from ucoslam_cv3_amd import UcoslamHipError

    pm, pnp = sc.fresh()
    good = [sc.true_c(), sc.wrong_c()]

    def refused(cands, objs=(pm, pnp), fr=None, **kw):
        from ucoslam_cv3_amd.relocalize import relocalize_pose_onecall

        args = dict(gates=GATES, n_keypoints=len(sc.fr["und_kpts"]))
        args.update(kw)
        isl = args.pop("isl", sc.inv_sf)
        with pytest.raises(UcoslamHipError):
            relocalize_pose_onecall(objs[0], objs[1], None, fr or sc.fr, cands, isl, MAX_DESC_DIST, **args)

    out = sc.true_c()
    out["matches"] = out["matches"].copy()
    out["matches"]["queryIdx"][3] = len(sc.fr["und_kpts"])
    refused([sc.wrong_c(), out])                                   # query_idx outside the frame
    neg = sc.true_c()
    neg["matches"] = neg["matches"].copy()
    neg["matches"]["queryIdx"][0] = -1
    refused([neg])
    refused(good, n_keypoints=10)                                  # capacities too small
    bad_s = sc.wrong_c()
    bad_s["samples"][7, 2] = 40
    refused([bad_s])                                               # a sample index outside the matches
    dup = sc.wrong_c()
    dup["samples"][5] = [1, 2, 2, 3]
    refused([dup])                                                 # an index twice in one sample
    refused(good, max_iters=0)
    refused(good, max_iters=1025)
    refused(good, fr=dict(sc.fr, fx=float("nan")))                 # non-finite intrinsics
    refused(good, isl=np.ones(17, np.float32))                     # n_levels beyond what the tracker takes
    refused(good * 33)                                             # more candidates than UH_RANSAC_MAX_PROBLEMS
    refused(good, objs=(sc.pm_host, sc.pnp_host))                  # a frame that is not device-resident
    _same(sc.composed(good), sc.onecall(good, objs=(pm, pnp)))     # the objects stay usable
