"""Pose-only PnP on an anisotropic, off-centre camera (fx, fy, cx, cy = 655.1, 742.3, 633.7, 171.4) against the real g2o (fixture
tests/golden/pnp_aniso_golden.npz): every other PnP input of the suite has fx == fy, so a solver that swaps them in a Jacobian row
or a projection passes there; here the reference itself moves by >= 1e-4 under that swap (the generator asserts it; 1.4 observed).
The CPU oracles against the fixture (CPU); the HIP solver's host and device entries, monocular and stereo (gpu).
Iterations, inliers and flags exact, se3 state within 1e-6."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import oracle_lib

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "pnp_aniso_golden.npz")
POSE_TOL = 1e-6


def _gen():
    spec = importlib.util.spec_from_file_location("make_pnp_aniso_golden", os.path.join(HERE, "golden", "make_pnp_aniso_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


GEN = _gen()
MONO, STEREO = list(GEN.MONO_CASES), list(GEN.STEREO_CASES)


def _golden():
    return np.load(GOLDEN)


def _assert_equals_reference(got, g, name, tol, label):
    iters = [int(i) for i in got["iters"]]
    dstate = np.abs(got["state"] - g[f"{name}_state"]).max()
    print(f"{name} [{label}]: iters {iters} ref {g[f'{name}_iters'].tolist()} ngood {int(got['ngood'])} ref {int(g[f'{name}_ngood'])} "
          f"|dstate| {dstate:.3e} flags differing {int((got['bad'] != g[f'{name}_bad']).sum())}")
    assert iters == g[f"{name}_iters"].tolist(), name
    assert int(got["ngood"]) == int(g[f"{name}_ngood"]), name
    np.testing.assert_array_equal(got["bad"], g[f"{name}_bad"], err_msg=name)
    assert dstate < tol, (name, dstate)
    assert np.abs(got["pose"] - g[f"{name}_pose"]).max() < 1e-5, name


# ------------------------------------------------------------------------------------------------ CPU
def test_problem_generator_reproduces_fixture_inputs():
    g = _golden()
    for name in MONO + STEREO:
        pr = GEN.problem(name)
        np.testing.assert_array_equal(GEN.input_digest(name, pr), g[f"{name}_in_digest"], err_msg=name)
        np.testing.assert_array_equal(pr["intr"], np.array(GEN.INTR, np.float32))
        assert len(g[f"{name}_bad"]) == pr["n"]
    assert GEN.INTR[0] != GEN.INTR[1] and max(GEN.MONO_CASES["mono3001"]["n"], 0) > 3000 and GEN.STEREO_CASES["mix3001"]["n"] > 3000
    mix = GEN.problem("mix500")
    assert 0.4 < (mix["depth"] > 0).mean() < 0.8


def test_default_camera_is_unchanged():
    """The optional intrinsics leave the default problem as it was (the other fixtures' digests depend on it)."""
    import synth

    a, b = synth.pnp_problem(300, 5), synth.pnp_problem(300, 5, intr=(718.856, 718.856, 607.19, 185.22))
    for k in ("pose", "intr", "p3d", "kp", "invsig", "weight"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_driver_regenerates_fixture_bit_for_bit():
    why = GEN.driver_available()
    if why is not None:
        pytest.skip(why)
    g = _golden()
    new = GEN.generate()
    assert sorted(new) == sorted(g.files)
    for k in g.files:
        np.testing.assert_array_equal(np.asarray(new[k]), g[k], err_msg=k)


@pytest.mark.parametrize("name", MONO + STEREO)
def test_cpu_oracle_equals_real_g2o(oracle, name):
    pr = GEN.problem(name)
    got = oracle_lib.pnp_solve(oracle, pr) if name in MONO else oracle_lib.pnp_solve_stereo(oracle, pr, pr["depth"], pr["bl"])
    _assert_equals_reference(got, _golden(), name, 1e-10, "oracle")


@pytest.mark.parametrize("name", ["mono500", "mix500"])
def test_fixture_discriminates_swapped_focal_lengths_without_the_reference(oracle, name):
    pr = GEN.swapped(GEN.problem(name))
    got = oracle_lib.pnp_solve(oracle, pr) if name in MONO else oracle_lib.pnp_solve_stereo(oracle, pr, pr["depth"], pr["bl"])
    move = np.abs(got["state"] - _golden()[f"{name}_state"]).max()
    print(f"{name} with fx <-> fy: state move {move:.3e}")
    assert move > 1e-4, (name, move)


# ------------------------------------------------------------------------------------------------ GPU
def _host(ctx, name):
    from ucoslam_cv3_amd.pnp import PnPSolver

    pr = GEN.problem(name)
    kw = dict(depth=pr["depth"], bl=pr["bl"]) if name in STEREO else {}
    sol = PnPSolver(ctx)
    got = sol.solvePnp(pr["pose"], pr["intr"], pr["p3d"], pr["kp"], pr["invsig"], pr["weight"], **kw)
    sol.close()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name", MONO + STEREO)
def test_hip_pnp_host_entry_equals_real_g2o(hip_ctx, name):
    _assert_equals_reference(_host(hip_ctx, name), _golden(), name, POSE_TOL, "host")


@pytest.mark.gpu
@pytest.mark.parametrize("name", MONO + STEREO)
def test_hip_pnp_dev_entry_equals_real_g2o(hip_ctx, name):
    import torch

    from ucoslam_cv3_amd._lib import check, lib
    from ucoslam_cv3_amd.pnp import PnPSolver

    pr = GEN.problem(name)
    n = pr["n"]
    keys = GEN.MONO_INPUT_KEYS + (("depth",) if name in STEREO else ())
    dev = {k: torch.from_numpy(np.ascontiguousarray(pr[k], np.float32)).cuda() for k in keys}
    work = torch.empty(n * 36, dtype=torch.uint8, device="cuda")
    pose_out = torch.zeros(16, dtype=torch.float32, device="cuda")
    bad = torch.zeros(n, dtype=torch.uint8, device="cuda")
    res = torch.zeros(5, dtype=torch.int32, device="cuda")
    state = torch.zeros(7, dtype=torch.float64, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    sol = PnPSolver(hip_ctx)
    torch.cuda.synchronize()
    common = (sol._h, ptr(dev["pose"]), ptr(dev["intr"]), n, ptr(dev["p3d"]), ptr(dev["kp"]), ptr(dev["invsig"]), ptr(dev["weight"]))
    outs = (ptr(work), ptr(pose_out), ptr(bad), ptr(res), ptr(state))
    if name in STEREO:
        check(lib().uh_pnp_solve_stereo_dev(*common, ptr(dev["depth"]), float(pr["bl"]), *outs))
    else:
        check(lib().uh_pnp_solve_dev(*common, *outs))
    hip_ctx.synchronize()
    r = res.cpu().numpy()
    got = dict(ngood=int(r[0]), iters=r[1:].tolist(), bad=bad.cpu().numpy(), state=state.cpu().numpy(), pose=pose_out.cpu().numpy())
    sol.close()
    _assert_equals_reference(got, _golden(), name, POSE_TOL, "dev")
    host = _host(hip_ctx, name)
    np.testing.assert_array_equal(got["state"], host["state"])           # the two entries run the same kernel
