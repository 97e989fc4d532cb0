"""Pose-only PnP with stereo / RGB-D observations (uh_pnp_solve_stereo, PnPSolver::solvePnp with Frame::getDepth > 0):
the HIP solver against the real g2o (fixture tests/golden/pnp_stereo_golden.npz), the device form, the monocular identity and the
argument checks (gpu); the fixture's inputs and its regeneration (CPU)."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import stereo_synth
import synth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "pnp_stereo_golden.npz")
POSE_TOL = 1e-6      # se3 state (unit quaternion + translation, fp64): the project's stated PnP tolerance


def _gen():
    spec = importlib.util.spec_from_file_location("make_pnp_stereo_golden", os.path.join(HERE, "golden", "make_pnp_stereo_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _golden():
    return np.load(GOLDEN)


# ------------------------------------------------------------------------------------------------ CPU
def test_problem_generator_reproduces_fixture_inputs():
    g, gen = _golden(), _gen()
    for name, kw in stereo_synth.CASES.items():
        pr = stereo_synth.stereo_pnp_problem(**kw)
        np.testing.assert_array_equal(gen.input_digest(pr), g[f"{name}_in_digest"], err_msg=name)
        assert len(g[f"{name}_bad"]) == kw["n"]


def test_fixture_covers_the_cases():
    g = _golden()
    mix = stereo_synth.stereo_pnp_problem(**stereo_synth.CASES["mix500"])
    assert 0.4 < (mix["depth"] > 0).mean() < 0.8 and mix["bad_depth"].any() and (mix["weight"] == 0.5).any()
    # grossly wrong depths are relabelled by the Chi3D test
    assert g["mix500_bad"][mix["bad_depth"]].mean() > 0.9
    assert (stereo_synth.stereo_pnp_problem(**stereo_synth.CASES["stereo800"])["depth"] > 0).all()
    assert (stereo_synth.stereo_pnp_problem(**stereo_synth.CASES["mono600"])["depth"] <= 0).all()
    assert int(g["early14_ngood"]) < 10 and g["early14_iters"][1:].tolist() == [0, 0, 0]
    assert stereo_synth.CASES["mix3001"]["n"] > 3000


def test_driver_regenerates_fixture_bit_for_bit():
    gen = _gen()
    why = gen.driver_available()
    if why is not None:
        pytest.skip(why)
    g = _golden()
    new = gen.generate()
    assert sorted(new) == sorted(g.files)
    for k in g.files:
        np.testing.assert_array_equal(np.asarray(new[k]), g[k], err_msg=k)


# ------------------------------------------------------------------------------------------------ GPU
def _solver(ctx):
    from ucoslam_cv3_amd.pnp import PnPSolver

    return PnPSolver(ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(stereo_synth.CASES))
def test_hip_stereo_matches_real_g2o(hip_ctx, name):
    g = _golden()
    pr = stereo_synth.stereo_pnp_problem(**stereo_synth.CASES[name])
    got = _solver(hip_ctx).solvePnp(pr["pose"], pr["intr"], pr["p3d"], pr["kp"], pr["invsig"], pr["weight"], depth=pr["depth"], bl=pr["bl"])
    assert got["iters"].tolist() == g[f"{name}_iters"].tolist()
    assert got["ngood"] == int(g[f"{name}_ngood"])
    np.testing.assert_array_equal(got["bad"], g[f"{name}_bad"])
    assert np.abs(got["state"] - g[f"{name}_state"]).max() < POSE_TOL
    assert np.abs(got["pose"] - g[f"{name}_pose"]).max() < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mix500", "mix3001"])
def test_hip_stereo_dev_form_equals_host_form(hip_ctx, name):
    import torch

    from ucoslam_cv3_amd._lib import check, lib

    pr = stereo_synth.stereo_pnp_problem(**stereo_synth.CASES[name])
    sol = _solver(hip_ctx)
    host = sol.solvePnp(pr["pose"], pr["intr"], pr["p3d"], pr["kp"], pr["invsig"], pr["weight"], depth=pr["depth"], bl=pr["bl"])
    n = len(pr["invsig"])
    dev = {k: torch.from_numpy(np.ascontiguousarray(pr[k], np.float32)).cuda() for k in stereo_synth.INPUT_KEYS}
    work = torch.empty(n * 36, dtype=torch.uint8, device="cuda")
    pose_out = torch.zeros(16, dtype=torch.float32, device="cuda")
    bad = torch.zeros(n, dtype=torch.uint8, device="cuda")
    res = torch.zeros(5, dtype=torch.int32, device="cuda")
    state = torch.zeros(7, dtype=torch.float64, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    torch.cuda.synchronize()
    check(lib().uh_pnp_solve_stereo_dev(sol._h, ptr(dev["pose"]), ptr(dev["intr"]), n, ptr(dev["p3d"]), ptr(dev["kp"]), ptr(dev["invsig"]),
                                        ptr(dev["weight"]), ptr(dev["depth"]), float(pr["bl"]), ptr(work), ptr(pose_out), ptr(bad), ptr(res), ptr(state)))
    hip_ctx.synchronize()
    r = res.cpu().numpy()
    assert int(r[0]) == host["ngood"] and r[1:].tolist() == host["iters"].tolist()
    np.testing.assert_array_equal(bad.cpu().numpy(), host["bad"])
    np.testing.assert_array_equal(state.cpu().numpy(), host["state"])
    np.testing.assert_array_equal(pose_out.cpu().numpy(), host["pose"])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [800, 1300, 3001])
def test_hip_stereo_without_depth_is_monocular_bit_for_bit(hip_ctx, n):
    pr = synth.pnp_problem(n, seed=n)
    sol = _solver(hip_ctx)
    args = (pr["pose"], pr["intr"], pr["p3d"], pr["kp"], pr["invsig"], pr["weight"])
    mono = sol.solvePnp(*args)
    rng = np.random.default_rng(n)
    no_depth = -rng.random(n).astype(np.float32) * (rng.random(n) < 0.5)   # zeros and negative depths: every match monocular
    for kw in (dict(depth=None, bl=0.54), dict(depth=no_depth, bl=0.54), dict(depth=np.zeros(n, np.float32), bl=0.0)):
        got = sol.solvePnp(*args, **kw)
        for k in ("pose", "bad", "iters", "state"):
            np.testing.assert_array_equal(got[k], mono[k], err_msg=k)
        assert got["ngood"] == mono["ngood"]


@pytest.mark.gpu
def test_hip_stereo_refuses_bad_arguments(hip_ctx):
    from ucoslam_cv3_amd._lib import lib, np_ptr

    pr = stereo_synth.stereo_pnp_problem(**stereo_synth.CASES["mix500"])
    sol = _solver(hip_ctx)
    with pytest.raises(Exception):
        sol.solvePnp(pr["pose"], pr["intr"], pr["p3d"], pr["kp"], pr["invsig"], pr["weight"], depth=pr["depth"], bl=0.0)
    with pytest.raises(Exception):
        sol.solvePnp(pr["pose"], pr["intr"], pr["p3d"], pr["kp"], pr["invsig"], pr["weight"], depth=pr["depth"], bl=-0.5)
    a = {k: np.ascontiguousarray(pr[k], np.float32) for k in stereo_synth.INPUT_KEYS}
    n = len(a["invsig"])
    pose, bad, it, st = np.zeros(16, np.float32), np.zeros(n, np.uint8), np.zeros(4, np.int32), np.zeros(7)
    L = lib()
    full = [sol._h, np_ptr(a["pose"]), np_ptr(a["intr"]), n, np_ptr(a["p3d"]), np_ptr(a["kp"]), np_ptr(a["invsig"]), np_ptr(a["weight"]),
            np_ptr(a["depth"]), C.c_float(0.54), np_ptr(pose), np_ptr(bad), np_ptr(it), np_ptr(st)]
    assert L.uh_pnp_solve_stereo(*full) >= 0   # the complete call succeeds
    for i in (0, 1, 2, 4, 5, 6, 7, 10, 11):   # NULL handle, pose, intrinsics, match arrays, outputs
        args = list(full)
        args[i] = None
        assert L.uh_pnp_solve_stereo(*args) < 0, i
    args = list(full)
    args[3] = -1
    assert L.uh_pnp_solve_stereo(*args) < 0
    # device form: a depth array without a baseline
    assert L.uh_pnp_solve_stereo_dev(sol._h, None, None, 0, None, None, None, None, None, C.c_float(0.5), None, None, None, None, None) < 0
    assert L.uh_pnp_solve_stereo_dev(sol._h, np_ptr(a["pose"]), np_ptr(a["intr"]), 0, None, None, None, None, np_ptr(a["depth"]), C.c_float(0.0),
                                     None, np_ptr(pose), None, np_ptr(it), None) < 0
