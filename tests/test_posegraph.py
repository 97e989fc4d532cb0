"""Loop-closure pose graph on the device (uh_posegraph_*; loopClosurePathOptimizationg2o, graphoptsim3.cpp:74-168) against the real g2o
(fixture tests/golden/posegraph_golden.npz, see tests/golden/make_posegraph_golden.py), through the C ABI on every case of
tests/posegraph_synth.py.

g2o differentiates the Sim3 edge numerically with a step of (double)1e-9f, which makes its own result irreproducible below ~1e-5, so the
optimiser is pinned twice: tightly with the step raised to 1e-4f on both sides, and at the reference's step as far as the reference pins
itself (ten times the spread its own state shows under 1e-12 jitters of the measurements, taken from the fixture).

pg12_big (rotation steps of 0.5 rad between keyframes, 0.15 rad and a 10 % scale jump at the closing edge) takes log()'s acos branch on
the closing edge from the first evaluation on and its general-sigma branches as soon as the scales move; with the 1e-4f step the
perturbed evaluations (|sigma| = 1e-4 > 1e-5, theta = 1e-4 > 1e-5) take the general branches of exp() and, for sigma, of log() as well.
At the reference's step every perturbation is below both thresholds, so that run exercises the small-angle / small-sigma branches."""
import os

import numpy as np
import pytest

import posegraph_synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "posegraph_golden.npz")
CASES = posegraph_synth.CASES
STEP = {"d4": np.float32(1e-4), "ref": np.float32(0.0)}
VAL_TOL = 1e-12     # errors and measurements carry no differencing noise
JAC_TOL = 1e-9      # the generator's SCREEN_TOL (1e-8 on the state after a whole optimisation) carried to one linearisation
STATE_TOL = 1e-6    # this project's BA / PnP bar
_cache = {}
_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = np.load(GOLDEN)
    return _golden


def problem(name):
    key = ("pr", name)
    if key not in _cache:
        _cache[key] = posegraph_synth.posegraph_problem(**CASES[name])
    return _cache[key]


def solve(pg, pr, step):
    out = pg.optimize(pr["poses"], pr["edge_i"], pr["edge_j"], pr["edge_w"] if len(pr["edge_w"]) else None, pr["idx_new"], pr["idx_old"], pr["expected"],
                      pr["fix_scale"], fd_delta=float(STEP[step]))
    out["lin"] = pg.debug_linearisation()
    return out


def run(hip_ctx, name, step):
    """Every (case, step) is optimised once per session, on one handle shared by all of them."""
    from ucoslam_cv3_amd.posegraph import PoseGraph

    if "pg" not in _cache:
        _cache["pg"] = PoseGraph(hip_ctx)
    key = (name, step)
    if key not in _cache:
        _cache[key] = solve(_cache["pg"], problem(name), step)
    return _cache[key]


def rel_chi2(out, info):
    got = np.array([out["chi2_before"], out["chi2_after"]])
    return float(np.abs(got - info[1:]).max() / (1 + np.abs(info[1:]).max()))


@pytest.mark.parametrize("name", list(CASES))
def test_first_linearisation_at_1e_4(hip_ctx, name):
    g, lin = golden(), run(hip_ctx, name, "d4")["lin"]
    d = {}
    for mine, ref in (("meas", "meas"), ("err", "lin_err")):
        want = g[f"{name}_d4_{ref}"]
        d[mine] = float((np.abs(lin[mine] - want) / (1 + np.abs(want))).max())
    for k in ("Ji", "Jj"):
        d[k] = float(np.abs(lin[k] - g[f"{name}_d4_lin_{k}"]).max())
    print(f"{name}: measurement {d['meas']:.2e} error {d['err']:.2e} (relative) Ji {d['Ji']:.2e} Jj {d['Jj']:.2e} (absolute)")
    assert d["meas"] <= VAL_TOL and d["err"] <= VAL_TOL
    assert d["Ji"] <= JAC_TOL and d["Jj"] <= JAC_TOL
    pr = problem(name)
    fixed_i, fixed_j = pr["edge_i"] == pr["idx_old"], pr["edge_j"] == pr["idx_old"]
    assert np.abs(lin["Ji"][fixed_i]).max(initial=0) == 0 and np.abs(lin["Jj"][fixed_j]).max(initial=0) == 0
    if pr["fix_scale"]:
        assert np.abs(lin["Ji"][:, :, 6]).max() == 0 and np.abs(lin["Jj"][:, :, 6]).max() == 0   # update[6] zeroed: both evaluations agree bit for bit


@pytest.mark.parametrize("name", list(CASES))
def test_optimisation_at_1e_4(hip_ctx, name):
    g, out = golden(), run(hip_ctx, name, "d4")
    want_it, info = int(g[f"{name}_d4_iters"][0]), g[f"{name}_d4_info"]
    ds = float(np.abs(out["state"] - g[f"{name}_d4_state"]).max())
    wp = g[f"{name}_d4_poses"]
    excess = float((np.abs(out["poses"].astype(np.float64) - wp) - STATE_TOL * (1 + np.abs(wp)) - np.spacing(np.abs(wp))).max())
    dc, bound_c = rel_chi2(out, info), 100 * float(g[f"{name}_d4_spread_chi2"])
    print(f"{name}: iterations {out['iterations']} / {want_it} trials {out['trials'].tolist()} / {g[f'{name}_d4_trials'][:want_it].tolist()} "
          f"state {ds:.2e} poses max {float(np.abs(out['poses'] - wp).max()):.2e} chi2 {dc:.2e} (bound {bound_c:.2e}) lambda {out['lambda_']:.3e} / {info[0]:.3e}")
    assert out["iterations"] == want_it
    assert ds <= STATE_TOL
    assert excess <= 0
    assert dc <= bound_c


@pytest.mark.parametrize("name", list(CASES))
def test_optimisation_at_reference_step(hip_ctx, name):
    g, out = golden(), run(hip_ctx, name, "ref")
    want_it, spread = int(g[f"{name}_ref_iters"][0]), float(g[f"{name}_ref_spread_state"])
    ds = float(np.abs(out["state"] - g[f"{name}_ref_state"]).max())
    print(f"{name}: iterations {out['iterations']} / {want_it} state {ds:.2e} = {ds / spread if spread else 0:.2f} x the reference's own spread {spread:.2e}")
    assert out["iterations"] == want_it
    assert ds <= 10 * spread


def test_fix_scale_keeps_every_scale_at_one(hip_ctx):
    for name, kw in CASES.items():
        for step in STEP:
            s = run(hip_ctx, name, step)["state"][:, 7]
            if kw["fix_scale"]:
                assert (s == 1.0).all(), (name, step)
    assert any(np.abs(run(hip_ctx, n, "d4")["state"][:, 7] - 1).max() > 1e-4 for n, kw in CASES.items() if not kw["fix_scale"])


def test_fixed_and_edgeless_poses_come_back_as_the_reference_returns_them(hip_ctx):
    g = golden()
    for name in CASES:
        pr, out = problem(name), run(hip_ctx, name, "ref")
        rows = [pr["idx_old"]] + ([pr["isolated"]] if pr["isolated"] >= 0 else [])
        for r in rows:   # the conversion round trip alone: identical up to the last bit of the normalisation
            assert np.abs(out["state"][r] - g[f"{name}_ref_state"][r]).max() <= 4e-16, (name, r)
            assert (np.abs(out["poses"][r] - g[f"{name}_ref_poses"][r]) <= np.spacing(np.abs(g[f"{name}_ref_poses"][r]))).all(), (name, r)
    pr = problem("pg12_mixed")
    assert pr["isolated"] >= 0 and not (pr["edge_i"] == pr["isolated"]).any() and not (pr["edge_j"] == pr["isolated"]).any()
    assert (pr["edge_i"] == pr["idx_old"]).sum() + (pr["edge_j"] == pr["idx_old"]).sum() >= 4   # the old keyframe has several edges


def test_smaller_problem_after_larger_on_one_handle_is_bit_identical(hip_ctx):
    from ucoslam_cv3_amd.posegraph import PoseGraph

    used, fresh = PoseGraph(hip_ctx), PoseGraph(hip_ctx)
    solve(used, problem("pg64_fixed"), "d4")
    a = solve(used, problem("pg5"), "d4")
    b = solve(used, problem("pg5"), "d4")
    c = solve(fresh, problem("pg5"), "d4")
    for other in (b, c):
        for k in ("poses", "state", "trials"):
            np.testing.assert_array_equal(a[k], other[k])
        assert (a["iterations"], a["lambda_"], a["chi2_before"], a["chi2_after"]) == (other["iterations"], other["lambda_"], other["chi2_before"], other["chi2_after"])
        for k in ("err", "Ji", "Jj", "meas"):
            np.testing.assert_array_equal(a["lin"][k], other["lin"][k])
    used.close(); fresh.close()


def test_graph_without_edges_returns_the_round_trip(hip_ctx):
    from ucoslam_cv3_amd.posegraph import PoseGraph

    pr = problem("pg5")
    pg = PoseGraph(hip_ctx)
    out = pg.optimize(pr["poses"], [], [], None, pr["idx_new"], pr["idx_old"], pr["expected"], 0)
    assert out["iterations"] == 0 and len(out["trials"]) == 0
    want = pr["poses"].copy()
    want[pr["idx_new"]] = pr["expected"]
    assert np.abs(out["poses"] - want).max() <= 2e-7 and (out["state"][:, 7] == 1).all()
    pg.close()


def test_refused_problems_launch_nothing(hip_ctx):
    from ucoslam_cv3_amd import UcoslamHipError
    from ucoslam_cv3_amd.posegraph import PoseGraph

    pr = problem("pg5")
    pg = PoseGraph(hip_ctx)
    bad_j = pr["edge_j"].copy()
    bad_j[1] = pr["n"]
    with pytest.raises(UcoslamHipError) as e:
        pg.optimize(pr["poses"], pr["edge_i"], bad_j, None, pr["idx_new"], pr["idx_old"], pr["expected"], 0)
    assert e.value.code == -1
    out = pg.optimize(pr["poses"], pr["edge_i"], pr["edge_j"], None, pr["idx_new"], pr["idx_old"], pr["expected"], 0, fd_delta=1e-4)   # the handle still works
    np.testing.assert_array_equal(out["state"], run(hip_ctx, "pg5", "d4")["state"])
    pg.close()
