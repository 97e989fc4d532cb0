"""Pose-only PnP on its rarely taken branches: the fixture tests/golden/pnp_hard_golden.npz (the real g2o on tests/pnp_hard_synth.py's
cases, every case screened against rounding noise) against its generator, the CPU oracle and its trace (CPU), and against the HIP solver
in every form (gpu)."""
import ctypes as C
import functools
import importlib.util
import os

import numpy as np
import pytest

import oracle_lib
import pnp_hard_synth as hs

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "pnp_hard_golden.npz")
STATE_TOL = 1e-6     # se3 state (unit quaternion + translation, fp64): the project's stated PnP tolerance
POSE_TOL = 1e-5      # the float pose matrix
ORACLE_TOL = 1e-10   # the CPU oracle against the real g2o, as tests/test_pnp.py
OUTPUTS = ("pose", "state", "bad", "iters")


def _gen():
    spec = importlib.util.spec_from_file_location("make_pnp_hard_golden", os.path.join(HERE, "golden", "make_pnp_hard_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@functools.lru_cache(maxsize=None)
def _golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


@functools.lru_cache(maxsize=None)
def _problem(name):
    return hs.case_problem(name)


@functools.lru_cache(maxsize=None)
def _trace(name):
    """The CPU oracle's outputs and trace of a case (computed once, shared, not modified)."""
    pr = _problem(name)
    return oracle_lib.pnp_trace(oracle_lib.load_oracle(), pr, pr["depth"], float(pr["bl"]))


def _ref(name):
    g = _golden()
    return {k: g[f"{name}_{k}"] for k in ("pose", "state", "bad", "ngood", "iters", "trials")}


def _distance(a, b):
    """max |a - b| over the finite entries; the non-finite ones must be the same values in the same places."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    fa, fb = np.isfinite(a), np.isfinite(b)
    np.testing.assert_array_equal(fa, fb, err_msg="non-finite entries in other places")
    np.testing.assert_array_equal(a[~fa], b[~fb], err_msg="other non-finite values")
    return float(np.abs(a[fa] - b[fb]).max()) if fa.any() else 0.0


# ------------------------------------------------------------------------------------------------ CPU
def test_problem_generator_reproduces_fixture_inputs():
    g, gen = _golden(), _gen()
    for name, case in hs.CASES.items():
        np.testing.assert_array_equal(gen.input_digest(_problem(name)), g[f"{name}_in_digest"], err_msg=name)
        assert len(g[f"{name}_bad"]) == case["n"] and g[f"{name}_trials"].shape == (4, 10)
    assert len(g) == 7 * len(hs.CASES)


def test_driver_regenerates_fixture_bit_for_bit_and_every_case_passes_the_screen():
    gen = _gen()
    why = gen.driver_available()
    if why is not None:
        pytest.skip(why)
    g = _golden()
    new = gen.generate()      # asserts the jitter screen on every case
    assert sorted(new) == sorted(g)
    for k in g:
        np.testing.assert_array_equal(np.asarray(new[k]), g[k], err_msg=k)


def test_oracle_trials_are_the_real_g2os():
    """The oracle's trials per iteration equal the recorded levenbergIterations entry for entry, and the trace is consistent in itself."""
    for name in hs.CASES:
        r, t = _ref(name), _trace(name)["trace"]
        np.testing.assert_array_equal(t["trials"], r["trials"], err_msg=name)
        for rd in range(4):
            it = int(r["iters"][rd])
            assert (r["trials"][rd, :it] >= 1).all() and (r["trials"][rd, it:] == 0).all(), name
            for i in range(it):
                acc, n_tr = int(t["accepted"][rd, i]), int(t["trials"][rd, i])
                assert acc in (-1, n_tr), (name, rd, i)                      # only an iteration's last trial can be the accepted one
                assert (t["reason"][rd, i] != 0) == (i == it - 1), (name, rd, i)   # a reason exactly where the round's iterations end
                assert bool(t["reason"][rd, i] & oracle_lib.PNP_TEN_TRIALS) == (n_tr == 10 and not t["lam_nonfinite"][rd, i]), (name, rd, i)


def test_fixture_covers_the_states():
    """Every state of pnp_hard_synth has a case that is in it, by the recorded iterations / trials / inliers and by the oracle's trace."""
    T = {name: _trace(name)["trace"] for name in hs.CASES}
    R = {name: _ref(name) for name in hs.CASES}
    states = {c["state"] for c in hs.CASES.values()}
    assert states == {hs.LARGE_STEP, hs.BOUNDARY, hs.BUDGET, hs.LOST, hs.BEHIND, hs.ZERO_INFORMATION, hs.PLANE_POINT, hs.HUGE_INFORMATION,
                      hs.LADDER_INSIDE, hs.LADDER_NINE, hs.LADDER_WALK, hs.LADDER_TEN}

    def iterations(name):
        return [(rd, i) for rd in range(4) for i in range(int(R[name]["iters"][rd]))]

    # large rotation steps, accepted, in a solve that converges; one LDS and both HBM forms, the largest LDS form, a stereo mix
    for name in hs.LARGE_STEP_CASES:
        assert T[name]["w2_accepted"].max() >= 0.25 and int(R[name]["ngood"]) >= 10, name
    shapes = {(hs.CASES[n]["n"], hs.CASES[n].get("stereo_frac", 0.0) > 0) for n in hs.LARGE_STEP_CASES}
    assert {(300, False), (3001, False), (3000, False), (400, True), (3001, True)} <= shapes
    mix = _problem("big_mix400")["depth"] > 0
    assert mix.any() and not mix.all() and (_problem("big_stereo3001")["depth"] > 0).all()
    # the ten-inlier rule: below ten matches a single round, from ten on all four; rounds that stop after the second and the third
    for n in (8, 9):
        assert R[f"n{n}"]["iters"][0] > 0 and R[f"n{n}"]["iters"][1:].tolist() == [0, 0, 0] and int(R[f"n{n}"]["ngood"]) == n
    for n in (10, 11):
        assert (R[f"n{n}"]["iters"] > 0).all() and int(R[f"n{n}"]["ngood"]) == n
    i2, i3 = R["stop_after_2"]["iters"], R["stop_after_3"]["iters"]
    assert i2[0] > 0 and i2[1] > 0 and i2[2:].tolist() == [0, 0] and int(R["stop_after_2"]["ngood"]) < 10
    assert (i3[:3] > 0).all() and i3[3] == 0 and int(R["stop_after_3"]["ngood"]) < 10
    # the budget: ten iterations, the tenth ended by the budget and not by Levenberg's Terminate
    terminate = oracle_lib.PNP_TEN_TRIALS | oracle_lib.PNP_RHO_ZERO | oracle_lib.PNP_LAMBDA_NONFINITE
    assert any(R["budget"]["iters"][rd] == 10 and T["budget"]["reason"][rd, 9] & oracle_lib.PNP_BUDGET and not T["budget"]["reason"][rd, 9] & terminate
               for rd in range(4))
    # lost: all outliers, a hopeless initial pose, everything behind the camera
    for name in ("lost_outliers", "lost_noise", "lost_behind"):
        assert int(R[name]["ngood"]) <= 3 and hs.CASES[name]["n"] >= 100, name
    assert len(_problem("lost_behind")["behind"]) == 100
    # 20 of 100 behind the camera: they are all outliers, the solve is not lost
    pb = _problem("behind20")
    assert len(pb["behind"]) == 20 and R["behind20"]["bad"][pb["behind"]].all() and int(R["behind20"]["ngood"]) >= 50
    # zero information: every factorisation of every round fails, ten trials, nothing is relabelled
    r, t = R["invsig0"], T["invsig0"]
    assert r["iters"].tolist() == [1, 1, 1, 1] and r["trials"][:, 0].tolist() == [10] * 4
    assert int(t["fails"].sum()) == 10 * 4 and (t["reason"][:, 0] == oracle_lib.PNP_TEN_TRIALS).all() and not r["bad"].any()
    # a point on the camera plane: lambda is not finite, the loop is left before its increment in every round
    r, t = R["plane_point"], T["plane_point"]
    assert r["iters"].tolist() == [1, 1, 1, 1] and r["trials"][:, 0].tolist() == [1] * 4
    assert (t["lam_nonfinite"][:, 0] == 1).all() and (t["reason"][:, 0] & oracle_lib.PNP_LAMBDA_NONFINITE).all() and int(t["fails"].sum()) == 0
    pp = _problem("plane_point")
    assert pp["p3d"][pp["plane_point"], 2] == 0 and (pp["pose"] == np.eye(4, dtype=np.float32).reshape(16)).all()
    # information 3e38: finite in the solver's doubles, the solve is lost in one round
    assert (_problem("invsig3e38")["invsig"] == np.float32(3e38)).all() and np.isfinite(R["invsig3e38"]["state"]).all()
    # the damping ladder, a monocular and a stereo case each
    for st, hit in ((hs.LADDER_INSIDE, lambda n_tr, acc: 2 <= n_tr <= 8 and acc == n_tr), (hs.LADDER_NINE, lambda n_tr, acc: n_tr == 9 and acc == 9),
                    (hs.LADDER_WALK, lambda n_tr, acc: n_tr == 10 and acc == -1), (hs.LADDER_TEN, lambda n_tr, acc: n_tr == 10 and acc == 10)):
        names = [n for n, c in hs.CASES.items() if c["state"] == st]
        assert {n in hs.MONO_CASES for n in names} == {True, False}, st
        for name in names:
            assert hs.CASES[name]["n"] <= 300
            assert any(hit(int(R[name]["trials"][rd, i]), int(T[name]["accepted"][rd, i])) for rd, i in iterations(name)), (st, name)
    for name in hs.CASES:
        assert (name in hs.MONO_CASES) == hs.is_mono(_problem(name)), name


def test_oracle_equals_real_g2o():
    worst = 0.0
    for name in hs.CASES:
        r, a = _ref(name), _trace(name)
        assert a["iters"].tolist() == r["iters"].tolist(), name
        assert int(a["ngood"]) == int(r["ngood"]), name
        np.testing.assert_array_equal(a["bad"], r["bad"], err_msg=name)
        d = _distance(a["state"], r["state"])
        worst = max(worst, d)
        assert d < ORACLE_TOL, (name, d)
        _distance(a["pose"], r["pose"])
    print(f"oracle vs real g2o: state differs by at most {worst:.2e}")


def _small_angle_oracle(name):
    pr = _problem(name)
    return oracle_lib.pnp_trace(oracle_lib.load_oracle(), pr, pr["depth"], float(pr["bl"]), small_angle_only=True)


def test_fixture_discriminates_the_large_rotation_branch():
    """An oracle whose SE3 exp keeps the small-angle constants at |omega| >= 0.5 misses the fixture's state on every large-step case by more
    than 100 x the GPU tolerance.

    Observed: 18.5 (big_mono3000) to 44.6 (big_mix400): the wrong oracle loses the solve in its first round, iterations [10, 0, 0, 0].
    That is what the large-step cases were chosen for (pnp_hard_synth.LARGE_STEP): at steps of |omega|^2 around 0.25 to 1 a solve that
    converges absorbs the wrong step and ends within 1e-7 of the right state, and only its path shows it (the next test)."""
    for name in hs.LARGE_STEP_CASES:
        wrong = _small_angle_oracle(name)
        d = float(np.abs(wrong["state"] - _ref(name)["state"]).max())
        print(f"{name}: the small-angle oracle misses the fixture's state by {d:.3e}, iterations {wrong['iters'].tolist()} against {_ref(name)['iters'].tolist()}")
        assert d > 100 * STATE_TOL, (name, d)


def test_wrong_large_rotation_branch_changes_the_recorded_trials():
    """The same wrong oracle misses the real g2o's trials per iteration and its iterations per round on every large-step case: the fixture
    pins the large-rotation branch through the path of the solve too, which the right oracle reproduces entry for entry
    (test_oracle_trials_are_the_real_g2os)."""
    n_iters = 0
    for name in hs.LARGE_STEP_CASES:
        wrong = _small_angle_oracle(name)
        assert not np.array_equal(wrong["trace"]["trials"], _ref(name)["trials"]), name
        n_iters += wrong["iters"].tolist() != _ref(name)["iters"].tolist()
    assert n_iters == len(hs.LARGE_STEP_CASES)


# ------------------------------------------------------------------------------------------------ GPU
def _solver(ctx):
    from ucoslam_cv3_amd.pnp import PnPSolver

    return PnPSolver(ctx)


def _solve(sol, pr, depth):
    return sol.solvePnp(pr["pose"], pr["intr"], pr["p3d"], pr["kp"], pr["invsig"], pr["weight"], depth=depth, bl=float(pr["bl"]))


def _same_bytes(a, b, what):
    for k in OUTPUTS:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)
    assert a["ngood"] == b["ngood"], what


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(hs.CASES))
def test_hip_matches_real_g2o(hip_ctx, name):
    """uh_pnp_solve / uh_pnp_solve_stereo against the fixture: iterations, inliers and flags identical, state within 1e-6, pose within 1e-5,
    non-finite outputs in the same places; a second call returns the same bytes; a monocular case through the stereo entry with no depth
    above zero returns the monocular entry's bytes.

    Observed on MI355X: iterations, inliers and flags identical in all 27 cases; |state - ref| at most 4.3e-13 (big_stereo3001; 6.7e-14
    big_mix400, 5.8e-14 lost_behind, below 1e-14 elsewhere), the float pose identical everywhere.  Before the solver took Eigen's
    failure rule and g2o's maximum for the initial lambda, plane_point came back with iterations [1, 0, 0, 0] against [1, 1, 1, 1]
    (ten failed trials at lambda = 0 and a relabelling at the input pose, where the reference leaves its loop on a non-finite lambda
    and relabels nothing)."""
    pr, r = _problem(name), _ref(name)
    sol = _solver(hip_ctx)
    mono = name in hs.MONO_CASES
    got = _solve(sol, pr, None if mono else pr["depth"])
    ds, dp = _distance(got["state"], r["state"]), _distance(got["pose"], r["pose"])
    print(f"{name}: iters {got['iters'].tolist()} ref {r['iters'].tolist()} ngood {got['ngood']} ref {int(r['ngood'])} "
          f"bad differ {int((got['bad'] != r['bad']).sum())} |state - ref| {ds:.2e} |pose - ref| {dp:.2e}")
    assert got["iters"].tolist() == r["iters"].tolist()
    assert got["ngood"] == int(r["ngood"])
    np.testing.assert_array_equal(got["bad"], r["bad"])
    assert ds < STATE_TOL and dp < POSE_TOL
    _same_bytes(_solve(sol, pr, None if mono else pr["depth"]), got, "second call")
    if mono:
        n = len(pr["invsig"])
        rng = np.random.default_rng(n)
        no_depth = -rng.random(n).astype(np.float32) * (rng.random(n) < 0.5)   # zeros and negative depths
        _same_bytes(_solve(sol, pr, no_depth), got, "stereo entry without a depth above zero")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["big_mono300", "big_mix400", "invsig0", "n8"])
def test_hip_dev_form_equals_host_form(hip_ctx, name):
    """uh_pnp_solve_dev (monocular cases) and uh_pnp_solve_stereo_dev byte for byte against the host entries."""
    import torch

    from ucoslam_cv3_amd._lib import check, lib

    pr = _problem(name)
    mono = name in hs.MONO_CASES
    sol = _solver(hip_ctx)
    host = _solve(sol, pr, None if mono else pr["depth"])
    n = len(pr["invsig"])
    dev = {k: torch.from_numpy(np.ascontiguousarray(pr[k], np.float32)).cuda() for k in hs.INPUT_KEYS}
    work = torch.empty(n * 36, dtype=torch.uint8, device="cuda")
    pose_out = torch.zeros(16, dtype=torch.float32, device="cuda")
    bad = torch.zeros(n, dtype=torch.uint8, device="cuda")
    res = torch.zeros(5, dtype=torch.int32, device="cuda")
    state = torch.zeros(7, dtype=torch.float64, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    torch.cuda.synchronize()
    common = (sol._h, ptr(dev["pose"]), ptr(dev["intr"]), n, ptr(dev["p3d"]), ptr(dev["kp"]), ptr(dev["invsig"]), ptr(dev["weight"]))
    outs = (ptr(work), ptr(pose_out), ptr(bad), ptr(res), ptr(state))
    if mono:
        check(lib().uh_pnp_solve_dev(*common, *outs))
    else:
        check(lib().uh_pnp_solve_stereo_dev(*common, ptr(dev["depth"]), float(pr["bl"]), *outs))
    hip_ctx.synchronize()
    r = res.cpu().numpy()
    got = dict(pose=pose_out.cpu().numpy(), state=state.cpu().numpy(), bad=bad.cpu().numpy(), iters=r[1:].copy(), ngood=int(r[0]))
    _same_bytes(got, host, "device form")
