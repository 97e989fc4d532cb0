"""Bundle adjustment: oracle vs real g2o (CPU), HIP vs oracle (gpu). Tolerances are stated in each assert."""
import numpy as np
import pytest

import oracle_lib
import synth

# fp64 everywhere; the only differences are summation order. Stated tolerance (BASELINE north_star "within a stated float
# tolerance"): final se3 pose state (unit quaternion + translation) within 1e-6 absolute; observed ~1e-12.
POSE_TOL = 1e-6


def _se3_rmse(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


def _assert_bad_flags_equal_up_to_the_boundary(got, ref, chi2_th=5.99):
    """Bad-association flags (chi2 > 5.99 or point behind the camera, globaloptimizer_g2o.cpp:497-521) must be IDENTICAL, except for
    an observation whose chi2 lies within the stated chi2 tolerance (1e-6 relative) of the 5.99 boundary itself — there the flag is
    decided by the last bits of a sum whose order differs between the two implementations."""
    diff = np.nonzero(got["bad"] != ref["bad"])[0]
    on_boundary = np.abs(ref["chi2"][diff] - chi2_th) <= 1e-6 * (1 + chi2_th)
    assert on_boundary.all(), f"{(~on_boundary).sum()} bad-association flags differ away from the chi2 = {chi2_th} boundary"


G2O_CASES = [(10, 3000, 0, 2), (6, 400, 1, 1), (4, 150, 2, 2), (10, 800, 3, 2)]
CHI2_TH, CHI2_NEAR = 5.99, 1e-3   # every chi2 within CHI2_NEAR of the threshold is recorded exactly (the boundary tolerance is 7e-6)


def _chi2_near_boundary(chi2):
    """The recorded part of chi2 that _assert_bad_flags_equal_up_to_the_boundary reads: the values within CHI2_NEAR of CHI2_TH."""
    near = np.nonzero(np.abs(chi2 - CHI2_TH) <= CHI2_NEAR)[0].astype(np.int32)
    return {"chi2_near_idx": near, "chi2_near": chi2[near]}


def _chi2_from_recording(rec, pre, n):
    """chi2 for the boundary check: the recorded values near CHI2_TH, NaN elsewhere (a flag that differs there fails the check, as it
    does with the full array: its chi2 lies more than CHI2_NEAR from the threshold)."""
    chi2 = np.full(n, np.nan)
    chi2[rec[pre + "chi2_near_idx"]] = rec[pre + "chi2_near"]
    return chi2


def g2o_ba_outputs(ref):
    """The real g2o's results on G2O_CASES (recorded in tests/golden/ref_outputs.npz, group g2o_ba).  chi2 is recorded as its largest
    magnitude, every value rounded to a multiple of half the stated tolerance 1e-6 (1 + max |chi2|), and exactly near the threshold."""
    out = {}
    for K, P, seed, nfix in G2O_CASES:
        b = oracle_lib.ba_optimize_ref(ref, synth.ba_problem(K, P, seed, nfixed=nfix), 5)
        pre = f"{K}_{P}_{seed}_{nfix}_"
        out.update({pre + f: b[f] for f in ("iters", "state", "points", "bad")})
        m = np.abs(b["chi2"]).max()
        out[pre + "chi2_max"] = np.array([m])
        out[pre + "chi2_q"] = np.rint(b["chi2"] / (1e-6 * (1 + m) / 2)).astype(np.int32)
        out.update({pre + k: v for k, v in _chi2_near_boundary(b["chi2"]).items()})
    return out


def g2o_ba_hard_outputs(ref):
    """The real g2o's results on synth.ba_hard_problem(0..15) (recorded in tests/golden/ref_outputs.npz, group g2o_ba_hard; of chi2
    the part the boundary check reads)."""
    out = {}
    for seed in range(16):
        b = oracle_lib.ba_optimize_ref(ref, synth.ba_hard_problem(seed), 5)
        out.update({f"s{seed}_{f}": b[f] for f in ("iters", "state", "bad")})
        out.update({f"s{seed}_{k}": v for k, v in _chi2_near_boundary(b["chi2"]).items()})
    return out


def test_oracle_matches_real_g2o(oracle):
    rec = oracle_lib.reference_outputs("g2o_ba", "g2o", g2o_ba_outputs)
    for K, P, seed, nfix in G2O_CASES:
        pr = synth.ba_problem(K, P, seed, nfixed=nfix)
        a = oracle_lib.ba_optimize(oracle, pr, 5)
        pre = f"{K}_{P}_{seed}_{nfix}_"
        b = {f: rec[pre + f] for f in ("iters", "state", "points", "bad")}
        b["chi2"] = _chi2_from_recording(rec, pre, len(b["bad"]))
        assert a["iters"].tolist() == b["iters"].tolist()
        assert np.abs(a["state"] - b["state"]).max() < 1e-9
        assert np.abs(a["points"] - b["points"]).max() < 1e-5
        # |a - chi2| <= |a - q step| + step / 2: the recorded rounding is added to the distance, so the stated bound still holds
        tol = 1e-6 * (1 + rec[pre + "chi2_max"][0])
        step = tol / 2
        assert (np.abs(a["chi2"] - rec[pre + "chi2_q"] * step) + step / 2).max() < tol
        _assert_bad_flags_equal_up_to_the_boundary(a, b)
        # and the optimisation did its job
        gt = pr["poses_gt"][:, :3, 3]
        err0 = np.abs(pr["poses"].reshape(-1, 4, 4)[:, :3, 3] - gt).max()
        err1 = np.abs(a["poses"].reshape(-1, 4, 4)[:, :3, 3] - gt).max()
        assert err1 < 0.35 * err0


def test_oracle_matches_real_g2o_where_trials_are_rejected(oracle):
    """The restated LM loop's OTHER branches against the real g2o: rejected trials (lambda *= ni, ni *= 2), the ten rejections in a row
    that terminate a pass, lambda factors other than 1/3, passes ended by the chi2 criterion — synth.ba_hard_problem produces all of
    them (the well-posed problems of the test above never leave the accept-by-1/3 branch).  Where pass 1 diverges so far that every
    edge is an outlier, g2o's second optimize() finds no active vertex and returns -1 without touching the state; the restatement
    counts that as one (empty) iteration: the states agree, the counts are compared where g2o reports one."""
    rec = oracle_lib.reference_outputs("g2o_ba_hard", "g2o", g2o_ba_hard_outputs)
    early = 0
    for seed in range(16):
        pr = synth.ba_hard_problem(seed)
        a = oracle_lib.ba_optimize(oracle, pr, 5)
        b = {f: rec[f"s{seed}_{f}"] for f in ("iters", "state", "bad")}
        b["chi2"] = _chi2_from_recording(rec, f"s{seed}_", len(b["bad"]))
        for ia, ib in zip(a["iters"].tolist(), b["iters"].tolist()):
            assert ib < 0 or ia == ib, (seed, a["iters"], b["iters"])
        assert np.abs(a["state"] - b["state"]).max() < 1e-8, (seed, np.abs(a["state"] - b["state"]).max())
        _assert_bad_flags_equal_up_to_the_boundary(a, b)
        early += a["iters"].tolist() != [5, 10]
    assert early >= 8


def test_oracle_golden_from_real_g2o(oracle):
    """Committed fixture generated from the real g2o (tests/golden/make_ba_golden.py): runs without /root/reference."""
    import os

    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "ba_golden.npz"))
    pr = {k[3:]: g[k] for k in g.files if k.startswith("in_")}
    pr["K"], pr["P"], pr["E"] = len(pr["fixed"]), len(pr["points"]), len(pr["obs_pt"])
    a = oracle_lib.ba_optimize(oracle, pr, 5)
    assert a["iters"].tolist() == g["ref_iters"].tolist()
    assert np.abs(a["state"] - g["ref_state"]).max() < 1e-9
    np.testing.assert_array_equal(a["bad"], g["ref_bad"])
    assert np.abs(a["points"] - g["ref_points"]).max() < 1e-5


def test_oracle_edge_jacobian_central_differences(oracle):
    """The analytic Jacobians of EdgeSE3ProjectXYZ (typesg2o.h:275-314) as the oracle evaluates them (oracle_ba_edge_eval = the
    function build_system calls) against central differences of computeError: d e / d X with X + h e_i, d e / d pose with
    exp(h e_i) * T (VertexSE3Expmap::oplusImpl: rotation components first, then translation)."""
    import ctypes as C

    VP = oracle_lib.VP
    oracle.oracle_ba_edge_eval.restype = None
    oracle.oracle_ba_edge_eval.argtypes = [VP] * 9
    P = oracle_lib.P
    rng = np.random.default_rng(5)

    def ev(pose, X, intr, uv, dpose=None, dX=None, jac=False):
        e, A, B = np.zeros(2), np.zeros(6), np.zeros(12)
        oracle.oracle_ba_edge_eval(P(pose), P(X), P(intr), P(uv), P(dpose) if dpose is not None else None, P(dX) if dX is not None else None,
                                   P(e), P(A) if jac else None, P(B) if jac else None)
        return e, A.reshape(2, 3), B.reshape(2, 6)

    worst = 0.0
    for _ in range(200):
        q = rng.standard_normal(4); q /= np.linalg.norm(q)
        if q[3] < 0:
            q = -q
        pose = np.r_[q, rng.uniform(-2, 2, 3)]
        Rm = np.array([[1 - 2 * (q[1] ** 2 + q[2] ** 2), 2 * (q[0] * q[1] - q[2] * q[3]), 2 * (q[0] * q[2] + q[1] * q[3])],
                       [2 * (q[0] * q[1] + q[2] * q[3]), 1 - 2 * (q[0] ** 2 + q[2] ** 2), 2 * (q[1] * q[2] - q[0] * q[3])],
                       [2 * (q[0] * q[2] - q[1] * q[3]), 2 * (q[1] * q[2] + q[0] * q[3]), 1 - 2 * (q[0] ** 2 + q[1] ** 2)]])
        pc = np.array([rng.uniform(-3, 3), rng.uniform(-2, 2), rng.uniform(2, 30)])      # in front of the camera
        X = Rm.T @ (pc - pose[4:])
        intr = np.array([718.856, 718.856, 607.19, 185.22])
        uv = rng.uniform(0, 1000, 2)
        e0, A, B = ev(pose, X, intr, uv, jac=True)
        h = 1e-6
        for i in range(3):
            d = np.zeros(3); d[i] = h
            num = (ev(pose, X, intr, uv, dX=d)[0] - ev(pose, X, intr, uv, dX=-d)[0]) / (2 * h)
            worst = max(worst, np.abs(num - A[:, i]).max() / (1 + np.abs(A[:, i]).max()))
        for i in range(6):
            d = np.zeros(6); d[i] = h
            num = (ev(pose, X, intr, uv, dpose=d)[0] - ev(pose, X, intr, uv, dpose=-d)[0]) / (2 * h)
            worst = max(worst, np.abs(num - B[:, i]).max() / (1 + np.abs(B[:, i]).max()))
    assert worst < 2e-6, worst          # central differences with h = 1e-6 in fp64: truncation ~h^2, round-off ~1e-10/h


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [(10, 3000, 0, 2), (6, 400, 1, 1), (4, 150, 2, 2), (12, 1500, 3, 3), (3, 60, 4, 3), (30, 1200, 5, 2), (22, 900, 6, 2), (14, 700, 7, 2),
                                 # the 16-lane persistent instantiation: 9 / 10 free keyframes (one row per lane in the solve), 11 / 13 / 16 (two rows per lane)
                                 (11, 3000, 8, 2), (12, 800, 9, 2), (13, 600, 10, 2), (15, 2500, 11, 2), (18, 1000, 12, 2), (18, 3000, 13, 2), (17, 40, 14, 1),
                                 # the launch chain's two-rows-per-lane solve at its limits: 17 and 21 free keyframes (127 rows)
                                 (19, 900, 15, 2), (23, 1100, 16, 2),
                                 # the stand-alone solve on a packed triangle in LDS: 22, 30, 31 and 32 (its limit) free keyframes; 33: the HBM workspace
                                 (24, 800, 17, 2), (32, 600, 18, 2), (33, 500, 19, 2), (34, 450, 20, 2), (35, 400, 21, 2),
                                 # the dense Schur form's remaining tile-row counts (10 at 25 free keyframes; 7-9, 11, 12 are above)
                                 (27, 700, 22, 2),
                                 # 33-64 free keyframes: the system in HBM, factorised by the same panels + MFMA update on global memory
                                 (42, 500, 23, 2), (50, 450, 24, 2), (66, 400, 25, 2)],
                         ids=lambda c: f"K{c[0]}_P{c[1]}_fix{c[3]}")
def test_hip_ba_matches_oracle(hip_ctx, oracle, cfg):
    from ucoslam_cv3_amd.ba import GlobalOptimizer, ParamSet

    K, P, seed, nfix = cfg
    pr = synth.ba_problem(K, P, seed, nfixed=nfix)
    opt = GlobalOptimizer.create(hip_ctx)
    opt.setParams(pr, ParamSet(nIters=5))
    opt.optimize()
    got = opt.getResults()
    ref = oracle_lib.ba_optimize(oracle, pr, 5)
    assert got["iters"].tolist() == ref["iters"].tolist()
    assert np.abs(got["state"] - ref["state"]).max() < POSE_TOL, np.abs(got["state"] - ref["state"]).max()
    assert _se3_rmse(got["state"], ref["state"]) < POSE_TOL
    assert np.abs(got["poses"] - ref["poses"]).max() < 1e-5          # float32 outputs
    assert np.abs(got["points"] - ref["points"]).max() < 1e-4
    assert np.abs(got["chi2"] - ref["chi2"]).max() < 1e-6 * (1 + np.abs(ref["chi2"]).max())
    _assert_bad_flags_equal_up_to_the_boundary(got, ref)
    # fixed frames come back untouched (getResults skips them)
    np.testing.assert_array_equal(got["poses"][pr["fixed"] == 1], pr["poses"][pr["fixed"] == 1])
    # re-running from the same snapshot is deterministic
    opt.optimize()
    again = opt.getResults()
    np.testing.assert_array_equal(again["state"], got["state"])
    assert len(opt.getBadAssociations()) == int(got["bad"].sum())


@pytest.mark.gpu
@pytest.mark.parametrize("K,P", [(6, 300), (14, 600), (24, 800), (30, 500)])
def test_hip_ba_chain_solve_in_hbm_at_small_sizes(hip_ctx, oracle, monkeypatch, K, P):
    """UH_BA_SOLVE=hbm + the launch chain forced (UH_BA_FORM=legacy): the HBM solve (33+ free keyframes in production) on systems of every
    small shape — an odd number of block columns, fewer rows than a wave, more than a tile row."""
    from ucoslam_cv3_amd.ba import GlobalOptimizer, ParamSet

    monkeypatch.setenv("UH_BA_SOLVE", "hbm")
    monkeypatch.setenv("UH_BA_FORM", "legacy")
    pr = synth.ba_problem(K, P, 40 + K, nfixed=1)
    ref = oracle_lib.ba_optimize(oracle, pr, 5)
    opt = GlobalOptimizer.create(hip_ctx)
    opt.setParams(pr, ParamSet(nIters=5))
    opt.optimize()
    got = opt.getResults()
    assert got["iters"].tolist() == ref["iters"].tolist()
    assert np.abs(got["state"] - ref["state"]).max() < POSE_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("K,P", [(19, 900), (26, 1100), (34, 450), (42, 400), (66, 300)])
def test_hip_ba_chain_schur_forms_agree(hip_ctx, oracle, monkeypatch, K, P):
    """17-64 free keyframes (fused, packed and HBM solve; the narrow and the wide dense kernel): the dense Schur form (MFMA product + reduce launch that leaves the finished system for the solve), the
    same with the solve assembling from the pair layout (UH_BA_PREBUILT=0) and the pair form (UH_BA_SCHUR_DENSE=0) all reproduce
    the oracle: same iteration counts, state within the tolerance."""
    from ucoslam_cv3_amd.ba import GlobalOptimizer, ParamSet

    pr = synth.ba_problem(K, P, 31 + K, nfixed=2)
    ref = oracle_lib.ba_optimize(oracle, pr, 5)
    states = []
    for env in ({}, {"UH_BA_PREBUILT": "0"}, {"UH_BA_SCHUR_DENSE": "0"}):
        for k in ("UH_BA_PREBUILT", "UH_BA_SCHUR_DENSE"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        opt = GlobalOptimizer.create(hip_ctx)
        opt.setParams(pr, ParamSet(nIters=5))
        opt.optimize()
        got = opt.getResults()
        assert opt.form() == "chain"
        assert got["iters"].tolist() == ref["iters"].tolist(), env
        assert np.abs(got["state"] - ref["state"]).max() < POSE_TOL, env
        states.append(got["state"])
    assert np.abs(states[0] - states[1]).max() < 1e-9 and np.abs(states[0] - states[2]).max() < 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [(10, 3000, 0, 2, True), (6, 400, 1, 1, True), (3, 60, 4, 2, True), (30, 1200, 5, 2, True), (14, 700, 7, 2, True),
                                 (80, 2500, 8, 2, False), (150, 4000, 9, 1, False)],
                         ids=lambda c: f"K{c[0]}_P{c[1]}_fix{c[3]}{'_forced' if c[4] else ''}")
def test_hip_ba_wide_form_matches_oracle(hip_ctx, oracle, cfg, monkeypatch):
    """The form for more than 64 free keyframes (global BA: sparse camera-pair lists, blocked dense LDL^T in HBM): forced on the
    small problems the other form solves (UH_BA_WIDE=1 is read by uh_ba_set_problem), and on 78 / 149 free keyframes."""
    from ucoslam_cv3_amd.ba import GlobalOptimizer, ParamSet

    K, P, seed, nfix, forced = cfg
    if forced:
        monkeypatch.setenv("UH_BA_WIDE", "1")
    pr = synth.ba_problem(K, P, seed, nfixed=nfix)
    opt = GlobalOptimizer.create(hip_ctx)
    opt.setParams(pr, ParamSet(nIters=5))
    opt.optimize()
    got = opt.getResults()
    ref = oracle_lib.ba_optimize(oracle, pr, 5)
    assert got["iters"].tolist() == ref["iters"].tolist()
    assert np.abs(got["state"] - ref["state"]).max() < POSE_TOL, np.abs(got["state"] - ref["state"]).max()
    assert np.abs(got["poses"] - ref["poses"]).max() < 1e-5
    assert np.abs(got["points"] - ref["points"]).max() < 1e-4
    _assert_bad_flags_equal_up_to_the_boundary(got, ref)
    np.testing.assert_array_equal(got["poses"][pr["fixed"] == 1], pr["poses"][pr["fixed"] == 1])
    opt.optimize()
    np.testing.assert_array_equal(opt.getResults()["state"], got["state"])


@pytest.mark.gpu
def test_hip_ba_stop_flag_and_errors(hip_ctx, oracle):
    import ucoslam_cv3_amd as u
    from ucoslam_cv3_amd.ba import GlobalOptimizer, ParamSet

    pr = synth.ba_problem(5, 200, 9)
    opt = GlobalOptimizer.create(hip_ctx)
    with pytest.raises(u.UcoslamHipError):          # optimize before setParams
        opt.optimize()
    opt.setParams(pr, ParamSet(nIters=5))
    stop = np.ones(1, np.uint8)                      # stopASAP already set: no iteration runs, poses unchanged
    opt.optimize(stop)
    got = opt.getResults()
    assert got["iters"].tolist() == [0, 0]
    assert np.abs(got["poses"] - pr["poses"]).max() < 1e-6
    with pytest.raises(RuntimeError):               # globaloptimizer.cpp:27-33
        GlobalOptimizer.create(hip_ctx, "ceres")
    bad = dict(pr)
    bad["obs_kf"] = pr["obs_kf"].copy()
    bad["obs_kf"][0] = 99
    with pytest.raises(u.UcoslamHipError):
        opt.setParams(bad)


@pytest.mark.gpu
def test_hip_ba_and_search_on_disjoint_compute_unit_shares(oracle):
    """uh_ctx_create_private_cus: the mapper's local BA on mask bits [0, 96) (12 CUs of every XCD on MI355X: the persistent form sizes its
    co-resident grid from the context's CU count), the tracker's search on the rest — same results as on the whole chip; a share that
    would leave an XCD empty, or reaches past the device, is refused."""
    import torch
    import ucoslam_cv3_amd as u
    from ucoslam_cv3_amd.ba import GlobalOptimizer, ParamSet
    from ucoslam_cv3_amd.knn import Index

    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    if ncu < 128:
        pytest.skip("needs a device with at least 128 compute units")
    ctx_ba, ctx_trk = u.Context(0, cus=(0, 96)), u.Context(0, cus=(96, ncu - 96))
    pr = synth.ba_problem(10, 3000, 0, nfixed=2)
    opt = GlobalOptimizer.create(ctx_ba)
    opt.setParams(pr, ParamSet(nIters=5))
    opt.optimize()
    got = opt.getResults()
    assert opt.form().startswith("persist")
    ref = oracle_lib.ba_optimize(oracle, pr, 5)
    assert got["iters"].tolist() == ref["iters"].tolist()
    assert np.abs(got["state"] - ref["state"]).max() < POSE_TOL
    train, q = synth.match_set(500, 3000, seed=5)
    idx, dist = Index(ctx_trk).build(torch.from_numpy(train).cuda()).search(torch.from_numpy(q).cuda(), 10)
    ctx_trk.synchronize()
    ri, rd = oracle_lib.knn_search(oracle, train, q, 10, 0)
    np.testing.assert_array_equal(idx.cpu().numpy(), ri)
    for bad in ((0, 4), (ncu - 8, 16), (-8, 16)):
        with pytest.raises(Exception):
            u.Context(0, cus=bad)


@pytest.mark.gpu
def test_hip_ba_async_equals_sync(hip_ctx):
    """uh_ba_optimize_async / uh_ba_wait (optimisation on the object's worker thread, like the reference's mapper thread)."""
    import ucoslam_cv3_amd as u
    from ucoslam_cv3_amd.ba import GlobalOptimizer, ParamSet

    pr = synth.ba_problem(6, 500, 11)
    opt = GlobalOptimizer.create(hip_ctx)
    opt.setParams(pr, ParamSet(nIters=5))
    with pytest.raises(u.UcoslamHipError):
        opt.wait()                               # nothing in flight
    opt.optimize()
    ref = opt.getResults()
    for _ in range(3):
        opt.optimize_async()
        with pytest.raises(u.UcoslamHipError):
            opt.optimize_async()                 # one optimisation in flight per object
        opt.wait()
        got = opt.getResults()
        np.testing.assert_array_equal(got["state"], ref["state"])
        assert got["iters"].tolist() == ref["iters"].tolist()


@pytest.mark.gpu
def test_hip_ba_persistent_exchange_tags_survive_the_sequence_wrap(hip_ctx, monkeypatch):
    """The persistent kernel's exchange words carry 20 bits of the optimizer's launch count; when they wrap the exchange region is zeroed
    again (ba.hip run_persistent).  An optimizer started three launches before the wrap (UH_BA_SEQ0) must give the same bytes on every
    one of eight optimisations across it, on the problem it was set up with and on a re-laid-out one."""
    import os

    from ucoslam_cv3_amd.ba import GlobalOptimizer, ParamSet

    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "ba_golden.npz"))
    pr_a = {k[3:]: g[k] for k in g.files if k.startswith("in_")}
    pr_b = synth.ba_problem(10, 1500, 3)

    def sig(opt):
        r = opt.getResults()
        return r["state"].tobytes() + r["iters"].tobytes() + r["bad"].tobytes() + r["chi2"].tobytes()

    ref = {}
    for name, pr in (("a", pr_a), ("b", pr_b)):
        opt = GlobalOptimizer.create(hip_ctx)
        opt.setParams(pr, ParamSet(nIters=5))
        opt.optimize()
        ref[name] = sig(opt)
    monkeypatch.setenv("UH_BA_SEQ0", str(0xFFFFF - 3))
    opt = GlobalOptimizer.create(hip_ctx)
    monkeypatch.delenv("UH_BA_SEQ0")
    opt.setParams(pr_a, ParamSet(nIters=5))
    for i in range(8):
        if i == 5:
            opt.setParams(pr_b, ParamSet(nIters=5))
        opt.optimize()
        assert sig(opt) == ref["a" if i < 5 else "b"], f"optimisation {i} after the tag wrap differs"


@pytest.mark.gpu
def test_hip_ba_persistent_is_exact_under_uneven_background_load(hip_ctx):
    """The persistent kernel's workgroup hand-offs and its LDS hygiene under UNEVEN load (scripts/ba_stress.py, shortened): problems with
    fewer free cameras than lane slots (6 of 8) and with all 8 are optimised repeatedly on a private stream while another stream
    keeps the chip busy with kNN searches and ORB extractions — other kernels' garbage in LDS, late and skewed workgroup arrivals.
    Every result must equal the unloaded one bit for bit.  (Round 2 found an uninitialised-LDS read exactly this way.)"""
    import os
    import threading
    import time

    import torch

    import ucoslam_cv3_amd as u
    from ucoslam_cv3_amd.ba import GlobalOptimizer, ParamSet
    from ucoslam_cv3_amd.knn import Index
    from ucoslam_cv3_amd.orb import FeatParams, ORBextractor

    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "ba_golden.npz"))
    problems = {"golden_6_free": {k[3:]: g[k] for k in g.files if k.startswith("in_")}, "8_free": synth.ba_problem(10, 1500, 3),
                "3_free": synth.ba_problem(5, 120, 4)}
    ctx_ba, ctx_bg = u.Context(0, private=True), u.Context(0, private=True)

    def run(pr):
        opt = GlobalOptimizer.create(ctx_ba)
        opt.setParams(pr, ParamSet(nIters=5))
        opt.optimize()
        r = opt.getResults()
        return r["state"].tobytes() + r["iters"].tobytes() + r["bad"].tobytes() + r["chi2"].tobytes()

    quiet = {k: run(p) for k, p in problems.items()}
    stop = []

    def background():
        torch.cuda.set_device(0)
        train, q = synth.match_set(2000, 10000, seed=0)
        index = Index(ctx_bg).build(torch.from_numpy(train).cuda())
        dq = torch.from_numpy(np.concatenate([q] * 4)).cuda()
        ext = ORBextractor.create(ctx_bg)
        frames = torch.from_numpy(np.stack([synth.frame(1241, 376, seed=s) for s in range(4)])).cuda()
        i = 0
        while not stop:
            if i % 3 == 0:
                time.sleep(0.0007 * (i % 5))
            index.search(dq, 10)
            ext.extract_batch(frames, FeatParams(2000, 8, 1.2))
            i += 1
        ctx_bg.synchronize()

    th = threading.Thread(target=background)
    th.start()
    try:
        time.sleep(2.0)                       # let the background reach steady state
        t0, n = time.time(), 0
        while time.time() - t0 < 6.0:
            for k, p in problems.items():
                assert run(p) == quiet[k], f"{k}: result under load differs from the unloaded one (run {n})"
                n += 1
        assert n > 100
    finally:
        stop.append(1)
        th.join()


@pytest.mark.gpu
def test_hip_ba_four_sessions_share_the_gpu_and_keep_their_results(hip_ctx):
    """Four independent sessions (an optimiser on a private context each) start their local BAs at the same moment: 4 x 94 spinning
    workgroups do not fit the persistent launches' admission budget (7/8 of the compute units, ba.hip PersistAdmission), so two run side
    by side and the others are admitted as those leave — none changes form, none times out, and every session's result equals the one
    it computes alone, bit for bit, round after round."""
    import ucoslam_cv3_amd as u
    from ucoslam_cv3_amd.ba import GlobalOptimizer, ParamSet

    def sig(opt):
        r = opt.getResults()
        return r["state"].tobytes() + r["iters"].tobytes() + r["bad"].tobytes()

    sessions = []
    for i in range(4):
        ctx = u.Context(0, private=True)
        opt = GlobalOptimizer.create(ctx)
        opt.setParams(synth.ba_problem(10, 3000, seed=300 + i), ParamSet(nIters=5))
        opt.optimize()
        sessions.append((ctx, opt, sig(opt)))
    assert all(opt.form().startswith("persist") for _, opt, _ in sessions)
    for rnd in range(25):
        for _, opt, _ in sessions:
            opt.optimize_async()
        for _, opt, _ in sessions:
            opt.wait()
        for i, (_, opt, alone) in enumerate(sessions):
            assert sig(opt) == alone, f"session {i}, round {rnd}: result beside three other sessions differs from the one computed alone"
        assert all(opt.form().startswith("persist") for _, opt, _ in sessions)


# ------------------------------------------------------------------------------------------------ the plugin protocol per keyframe
def _sig(r):
    return r["state"].tobytes() + r["iters"].tobytes() + r["bad"].tobytes() + r["chi2"].tobytes() + r["poses"].tobytes() + r["points"].tobytes()


@pytest.mark.gpu
def test_hip_ba_fresh_problem_per_keyframe(hip_ctx, oracle):
    """A local BA is a NEW problem per keyframe (mapmanager.cpp:11388-11405 setParams + optimize, :1267-1305 getResults): ONE optimizer
    object takes a stream of different windows — sizes growing and shrinking, persistent form and launch chain alternating, staging
    blocks regrown, the (point x frame) table reused without clearing — and every result equals a fresh object's result on the
    same problem bit for bit, and the oracle within the stated tolerance."""
    from ucoslam_cv3_amd.ba import GlobalOptimizer, ParamSet

    stream = [(10, 3000, 0, 2), (6, 400, 1, 1), (12, 1500, 3, 3), (10, 3000, 5, 2), (20, 700, 9, 2), (4, 150, 2, 2), (10, 3400, 7, 2), (9, 900, 8, 1),
              (18, 1200, 6, 2), (5, 33, 5, 2), (10, 3000, 0, 2)]
    opt = GlobalOptimizer.create(hip_ctx)
    forms = []
    for K, P, seed, nfix in stream:
        pr = synth.ba_problem(K, P, seed, nfixed=nfix)
        opt.setParams(pr, ParamSet(nIters=5))
        forms.append(opt.form())
        opt.optimize()
        got = opt.getResults()
        fresh = GlobalOptimizer.create(hip_ctx)
        fresh.setParams(pr, ParamSet(nIters=5))
        fresh.optimize()
        assert _sig(fresh.getResults()) == _sig(got), f"problem {(K, P, seed, nfix)} in the stream differs from a fresh optimizer"
        ref = oracle_lib.ba_optimize(oracle, pr, 5)
        assert got["iters"].tolist() == ref["iters"].tolist()
        assert np.abs(got["state"] - ref["state"]).max() < POSE_TOL
        _assert_bad_flags_equal_up_to_the_boundary(got, ref)
    assert "persist8" in forms and "persist16" in forms and "chain" in forms


@pytest.mark.gpu
def test_hip_ba_staged_protocol_equals_array_protocol(hip_ctx):
    """uh_ba_map_staging / uh_ba_set_problem_staged / uh_ba_results_view_get (no host copy on either side) against
    uh_ba_set_problem / uh_ba_get_results on the same problems, incl. a window the persistent form does not take (staged -> tables)."""
    from ucoslam_cv3_amd.ba import GlobalOptimizer, ParamSet

    a, b = GlobalOptimizer.create(hip_ctx), GlobalOptimizer.create(hip_ctx)
    for K, P, seed, nfix in [(10, 3000, 0, 2), (7, 500, 3, 1), (10, 3000, 4, 2), (13, 800, 5, 2)]:
        pr = synth.ba_problem(K, P, seed, nfixed=nfix)
        a.setParams(pr, ParamSet(nIters=5)); a.optimize()
        want = a.getResults()
        dims = b.fillStaging(pr)
        b.setParamsStaged(*dims, ParamSet(nIters=5)); b.optimize()
        got = b.getResults()
        assert _sig(got) == _sig(want)
        if b.form().startswith("persist"):
            v = b.resultsView()
            for k in ("poses", "points", "chi2", "bad", "state", "iters"):
                np.testing.assert_array_equal(v[k], want[k])


@pytest.mark.gpu
def test_hip_ba_duplicate_and_out_of_range_observations(hip_ctx):
    """A (point, frame) pair that occurs twice is found by the ingest kernel and reported by optimize(); an index out of range is
    refused by setParams itself (both entry points); the object stays usable."""
    import ucoslam_cv3_amd as u
    from ucoslam_cv3_amd.ba import GlobalOptimizer, ParamSet

    pr = synth.ba_problem(6, 300, 2)
    opt = GlobalOptimizer.create(hip_ctx)
    dup = dict(pr)
    for k in ("obs_pt", "obs_kf", "obs_uv", "obs_w"):
        dup[k] = np.concatenate([pr[k], pr[k][17:18]])
    dup["E"] = pr["E"] + 1
    opt.setParams(dup, ParamSet(nIters=5))
    with pytest.raises(u.UcoslamHipError, match="observed twice"):
        opt.optimize()
    bad = dict(pr)
    bad["obs_pt"] = pr["obs_pt"].copy(); bad["obs_pt"][5] = pr["P"]
    with pytest.raises(u.UcoslamHipError, match="out of range"):
        opt.setParams(bad)
    dims = opt.fillStaging(bad)
    with pytest.raises(u.UcoslamHipError, match="out of range"):
        opt.setParamsStaged(*dims)
    opt.setParams(pr, ParamSet(nIters=5)); opt.optimize()
    fresh = GlobalOptimizer.create(hip_ctx)
    fresh.setParams(pr, ParamSet(nIters=5)); fresh.optimize()
    assert _sig(opt.getResults()) == _sig(fresh.getResults())


@pytest.mark.gpu
def test_hip_ba_solve_async_runs_setparams_and_optimize_on_the_worker(hip_ctx):
    """uh_ba_solve_async: the mapper thread's two calls (setParams + optimize) on the object's worker; getResults on the caller's thread."""
    from ucoslam_cv3_amd.ba import GlobalOptimizer, ParamSet

    opt, ref = GlobalOptimizer.create(hip_ctx), GlobalOptimizer.create(hip_ctx)
    ps = ParamSet(nIters=5)
    for seed in range(4):
        pr = synth.ba_problem(10, 1200 + 200 * seed, seed)
        ref.setParams(pr, ps); ref.optimize()
        want = _sig(ref.getResults())
        opt.solve_async(pr, ps)
        opt.wait()
        assert _sig(opt.getResults()) == want
        dims = opt.fillStaging(pr)
        opt.solve_async(None, ps, dims=dims)
        opt.wait()
        assert _sig(opt.getResults()) == want


@pytest.mark.gpu
def test_hip_ba_table_sequence_wrap(hip_ctx):
    """The (point x frame) table is never cleared between problems: its cells carry 12 bits of problem sequence.  4100 setParams on one
    object cross the wrap (the table is zeroed there); a problem whose cells were written 4095 problems earlier must not be seen."""
    from ucoslam_cv3_amd.ba import GlobalOptimizer, ParamSet

    small = synth.ba_problem(5, 40, 1)
    big = synth.ba_problem(8, 300, 2)
    opt, fresh = GlobalOptimizer.create(hip_ctx), GlobalOptimizer.create(hip_ctx)
    fresh.setParams(big, ParamSet(nIters=5)); fresh.optimize()
    want = _sig(fresh.getResults())
    opt.setParams(big, ParamSet(nIters=5))
    for i in range(4100):
        opt.setParams(small, ParamSet(nIters=2))
        if i % 1024 == 1023:
            opt.optimize()
    opt.setParams(big, ParamSet(nIters=5)); opt.optimize()
    assert _sig(opt.getResults()) == want


@pytest.mark.gpu
def test_hip_ba_compact_and_full_observation_records_agree(hip_ctx, monkeypatch):
    """uh_ba_set_problem sends 16-byte records {point | frame << 24, u, v, (float)inv_sigma} when every information scalar is float-exact
    (a third fewer bytes over the host link) and 24-byte records otherwise: same results bit for bit; a problem with ONE inexact scalar
    takes the 24-byte form by itself."""
    from ucoslam_cv3_amd.ba import GlobalOptimizer, ParamSet

    for cfg in ((10, 3000, 0, 2), (13, 901, 4, 2), (5, 77, 2, 1)):
        pr = synth.ba_problem(*cfg[:3], nfixed=cfg[3])
        sigs = []
        for force24 in (False, True):
            if force24:
                monkeypatch.setenv("UH_BA_OBS24", "1")
            else:
                monkeypatch.delenv("UH_BA_OBS24", raising=False)
            opt = GlobalOptimizer.create(hip_ctx)
            opt.setParams(pr, ParamSet(nIters=5))
            opt.optimize()
            sigs.append(_sig(opt.getResults()))
        assert sigs[0] == sigs[1]
        monkeypatch.delenv("UH_BA_OBS24", raising=False)
        # the packing loop has an AVX-512 form (eight records per step) and an SSE form (two): same records, also where an index is out of range
        monkeypatch.setenv("UH_BA_NO_AVX512", "1")
        opt = GlobalOptimizer.create(hip_ctx)
        opt.setParams(pr, ParamSet(nIters=5))
        opt.optimize()
        assert _sig(opt.getResults()) == sigs[0]
        monkeypatch.delenv("UH_BA_NO_AVX512", raising=False)
        if cfg[1] > 100:
            bad = dict(pr)
            bad["obs_pt"] = pr["obs_pt"].copy()
            bad["obs_pt"][11] = cfg[1] + 5
            with pytest.raises(Exception):
                GlobalOptimizer.create(hip_ctx).setParams(bad, ParamSet(nIters=5))
        odd = dict(pr)
        odd["obs_w"] = pr["obs_w"].copy()
        odd["obs_w"][len(odd["obs_w"]) // 2] = 1.0 / 3.0          # not a float: the whole problem goes out as 24-byte records
        a, b = GlobalOptimizer.create(hip_ctx), GlobalOptimizer.create(hip_ctx)
        a.setParams(odd, ParamSet(nIters=5)); a.optimize()
        monkeypatch.setenv("UH_BA_OBS24", "1")
        b.setParams(odd, ParamSet(nIters=5)); b.optimize()
        monkeypatch.delenv("UH_BA_OBS24", raising=False)
        assert _sig(a.getResults()) == _sig(b.getResults())


@pytest.mark.gpu
def test_hip_ba_chi2_handover_can_be_switched_off(hip_ctx):
    """uh_ba_want_chi2(0): the kernel's tail leaves the per-observation chi2 (an extra of this ABI) out of its result hand-over; everything
    the reference's getResults returns is unchanged, asking for chi2 is an error, switching it back on works."""
    import ucoslam_cv3_amd as u
    from ucoslam_cv3_amd._lib import check, np_ptr
    from ucoslam_cv3_amd.ba import GlobalOptimizer, ParamSet

    pr = synth.ba_problem(10, 1500, 3)
    ref = GlobalOptimizer.create(hip_ctx)
    ref.setParams(pr, ParamSet(nIters=5)); ref.optimize()
    want = ref.getResults()
    opt = GlobalOptimizer.create(hip_ctx).wantChi2(False)
    opt.setParams(pr, ParamSet(nIters=5)); opt.optimize()
    poses, points, bad, iters = np.zeros((pr["K"], 16), np.float32), np.zeros((pr["P"], 3), np.float32), np.zeros(pr["E"], np.uint8), np.zeros(2, np.int32)
    check(u.lib().uh_ba_get_results(opt._h, np_ptr(poses), np_ptr(points), None, np_ptr(bad), np_ptr(iters)))
    np.testing.assert_array_equal(poses, want["poses"]); np.testing.assert_array_equal(points, want["points"])
    np.testing.assert_array_equal(bad, want["bad"]); assert iters.tolist() == want["iters"].tolist()
    with pytest.raises(u.UcoslamHipError, match="chi2 was switched off"):
        opt.getResults()
    opt.wantChi2(True)
    opt.setParams(pr, ParamSet(nIters=5)); opt.optimize()
    assert _sig(opt.getResults()) == _sig(want)


@pytest.mark.gpu
def test_hip_ba_hard_problems_rejected_trials_and_other_lambda_factors(hip_ctx, oracle):
    """Local BAs that Levenberg-Marquardt does not sail through (synth.ba_hard_problem: rejected trials up to the ten in a row that end a
    pass, accepted trials with lambda factors other than 1/3, passes cut short by the chi2 criterion).  The persistent kernel's
    speculative trials (phase 1 of the next trial with lambda / 3 before the decision) must be DROPPED in exactly those cases: same
    iteration counts and state as the oracle, and the debug counters show that both outcomes occurred over the set."""
    import ctypes as C
    from ucoslam_cv3_amd.ba import GlobalOptimizer, ParamSet
    import ucoslam_cv3_amd as u

    L = u.lib()
    L.uh_ba_debug_clocks.argtypes = [C.c_void_p, C.c_void_p]; L.uh_ba_debug_clocks.restype = C.c_int
    kept = dropped = early = 0
    for seed in range(16):
        pr = synth.ba_hard_problem(seed)
        ref = oracle_lib.ba_optimize(oracle, pr, 5)
        opt = GlobalOptimizer.create(hip_ctx)
        opt.setParams(pr, ParamSet(nIters=5))
        opt.optimize()
        got = opt.getResults()
        assert got["iters"].tolist() == ref["iters"].tolist(), seed
        assert np.abs(got["state"] - ref["state"]).max() < POSE_TOL, (seed, np.abs(got["state"] - ref["state"]).max())
        _assert_bad_flags_equal_up_to_the_boundary(got, ref)
        early += ref["iters"].tolist() != [5, 10]
        assert opt.form().startswith("persist")
        clk = np.zeros(64, dtype=np.int64)
        assert L.uh_ba_debug_clocks(opt._h, clk.ctypes.data) == 0
        kept += int(clk[58]); dropped += int(clk[59])
        opt.close()
    assert early >= 4            # the set does contain passes that end before their iteration budget
    assert kept > 0 and dropped > 0, (kept, dropped)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [(10, 3000, 0, 2), (18, 1000, 12, 2), (6, 400, 1, 1)], ids=lambda c: f"K{c[0]}_P{c[1]}")
def test_hip_ba_speculative_and_plain_trials_agree(hip_ctx, oracle, cfg, monkeypatch):
    """UH_BA_SPEC=0 keeps the three-hand-off trial (errors, chi2 hand-off, decision; the form every pass's LAST trial takes anyway) for the
    whole optimisation: same iteration counts, states equal to round-off (the chi2 sums are added in another order), both within the
    tolerance of the oracle."""
    from ucoslam_cv3_amd.ba import GlobalOptimizer, ParamSet

    K, P, seed, nfix = cfg
    pr = synth.ba_problem(K, P, seed, nfixed=nfix)
    ref = oracle_lib.ba_optimize(oracle, pr, 5)
    res = {}
    for spec in ("1", "0"):
        monkeypatch.setenv("UH_BA_SPEC", spec)
        opt = GlobalOptimizer.create(hip_ctx)
        opt.setParams(pr, ParamSet(nIters=5))
        opt.optimize()
        res[spec] = opt.getResults()
        opt.close()
        assert res[spec]["iters"].tolist() == ref["iters"].tolist()
        assert np.abs(res[spec]["state"] - ref["state"]).max() < POSE_TOL
    assert np.abs(res["1"]["state"] - res["0"]["state"]).max() < 1e-11
    np.testing.assert_array_equal(res["1"]["bad"], res["0"]["bad"])


@pytest.mark.gpu
@pytest.mark.parametrize("staged", [False, True], ids=["arrays", "staged"])
def test_hip_ba_falls_back_to_the_launch_chain_when_the_persistent_kernel_cannot_become_resident(hip_ctx, oracle, monkeypatch, staged):
    """The persistent form needs all its workgroups resident at once; when another spinning kernel holds CUs (a second process on the
    GPU), its launch gives up after a timeout.  optimize() must then not fail: the problem is still in the staging block (either record
    format), so this optimisation and the object's next problems take the launch chain (UH_BA_FAIL_RESIDENCY=1 forces the failure)."""
    from ucoslam_cv3_amd.ba import GlobalOptimizer, ParamSet

    pr = synth.ba_problem(10, 800, 3, nfixed=2)
    ref = oracle_lib.ba_optimize(oracle, pr, 5)
    opt = GlobalOptimizer.create(hip_ctx)
    def set_():
        if staged:
            dims = opt.fillStaging(pr)
            opt.setParamsStaged(*dims, ParamSet(nIters=5))
        else:
            opt.setParams(pr, ParamSet(nIters=5))
    set_()
    assert opt.form() == "persist8"
    monkeypatch.setenv("UH_BA_FAIL_RESIDENCY", "1")
    opt.optimize()                               # falls back instead of raising
    monkeypatch.delenv("UH_BA_FAIL_RESIDENCY")
    assert opt.form() == "chain"
    got = opt.getResults()
    assert got["iters"].tolist() == ref["iters"].tolist()
    assert np.abs(got["state"] - ref["state"]).max() < POSE_TOL
    _assert_bad_flags_equal_up_to_the_boundary(got, ref)
    set_()                                       # the next problems of this object stay on the chain for a while ...
    assert opt.form() == "chain"
    opt.optimize()
    assert np.abs(opt.getResults()["state"] - ref["state"]).max() < POSE_TOL
    for _ in range(70):                          # ... and then the persistent form is tried again
        set_()
    assert opt.form() == "persist8"
    opt.optimize()
    assert np.abs(opt.getResults()["state"] - ref["state"]).max() < POSE_TOL
    if staged:   # a caller that has already remapped the staging block (for the next keyframe) cannot be served by the fallback: refused, not guessed
        from ucoslam_cv3_amd._lib import UcoslamHipError

        set_()
        opt.fillStaging(pr)
        monkeypatch.setenv("UH_BA_FAIL_RESIDENCY", "1")
        with pytest.raises(UcoslamHipError, match="remapped"):
            opt.optimize()
        monkeypatch.delenv("UH_BA_FAIL_RESIDENCY")
    opt.close()
