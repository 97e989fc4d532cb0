"""Pose-only PnP with marker observations (uh_pnp_solve_markers, PnPSolver::solvePnp with frame.markers, pnpsolver.cpp:280-386):
the HIP solver against the real g2o (fixture tests/golden/pnp_marker_golden.npz, every case screened against the reference's own
float-rounding discontinuities, see tests/golden/make_pnp_marker_golden.py), the device form, the marker-free identity and the argument
checks (gpu); the fixture's inputs, the branches it covers and its regeneration (CPU)."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

import marker_synth
import stereo_synth
import synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "pnp_marker_golden.npz")
POSE_TOL = 1e-6      # se3 state (unit quaternion + translation, fp64): the project's stated PnP tolerance
CASES = marker_synth.CASES


def _gen():
    spec = importlib.util.spec_from_file_location("make_pnp_marker_golden", os.path.join(HERE, "golden", "make_pnp_marker_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _golden():
    return np.load(GOLDEN)


def _problem(name):
    return marker_synth.marker_pnp_problem(**CASES[name])


# ------------------------------------------------------------------------------------------------ CPU
def test_problem_generator_reproduces_fixture_inputs():
    g, gen = _golden(), _gen()
    for name, kw in CASES.items():
        pr = _problem(name)
        np.testing.assert_array_equal(gen.input_digest(pr), g[f"{name}_in_digest"], err_msg=name)
        assert len(g[f"{name}_bad"]) == kw["n"] and len(pr["markers"]["size"]) == kw["n_markers"]
        assert pr["markers"]["pose_g2m"].dtype == np.float32 and pr["markers"]["und_corners"].shape == (kw["n_markers"], 8)


def test_fixture_covers_the_branches():
    g = _golden()
    it = {name: g[f"{name}_iters"].tolist() for name in CASES}
    shape = {name: (kw["n"], kw["n_markers"]) for name, kw in CASES.items()}
    assert sorted(shape.values()) == sorted([(300, 2), (40, 1), (5, 2), (300, 2), (0, 1), (0, 2), (300, 2), (500, 3), (3001, 3), (300, 0)])
    # below the 10-inlier stop, which must not fire with markers
    assert int(g["kp5_m2_ngood"]) < 10 and all(v > 0 for v in it["kp5_m2"])
    assert int(g["out97_m2_ngood"]) < 10 and all(v > 0 for v in it["out97_m2"])
    assert synth.pnp_problem(**{k: v for k, v in CASES["out97_m2"].items() if k != "n_markers"})["outlier"].mean() > 0.95
    # marker-only, inf weight: started far, round 0 makes one rejected trial and the kernel goes by the chi2 rule; started close, the
    # kernel survives three rounds of one rejected trial each until the round rule removes it
    assert it["m1_far"][0] == 1 and all(v > 1 for v in it["m1_far"][1:])
    assert it["m2_close"][:3] == [1, 1, 1] and it["m2_close"][3] > 1
    for name in ("m1_far", "m2_close"):
        pr = _problem(name)
        assert int(g[f"{name}_ngood"]) == 0
        moved = np.abs(g[f"{name}_pose"] - pr["pose"]).max()
        assert moved > 0, name   # the rejected trials leave the pose alone; the kernel-free rounds move it
    # ~30 px corner noise: far above Chi8D at any pose
    assert CASES["noisy_m2"]["corner_noise"] >= 30
    mix = _problem("mix500_m3")
    assert 0.4 < (mix["depth"] > 0).mean() < 0.8
    assert CASES["kp3001_m3"]["n"] > 3000
    assert np.isfinite(np.concatenate([g[f"{n}_state"] for n in CASES])).all()


def test_driver_regenerates_fixture_bit_for_bit_and_every_case_passes_the_screen():
    gen = _gen()
    why = gen.driver_available()
    if why is not None:
        pytest.skip(why)
    g = _golden()
    new = gen.generate()   # (asserts the jitter screen for every case)
    assert sorted(new) == sorted(g.files)
    for k in g.files:
        np.testing.assert_array_equal(np.asarray(new[k]), g[k], err_msg=k)
    # no markers: the driver is the stereo fixture's driver (the monocular behaviour)
    spec = importlib.util.spec_from_file_location("make_pnp_stereo_golden", os.path.join(HERE, "golden", "make_pnp_stereo_golden.py"))
    st = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(st)
    pr = _problem("kp300_m0")
    ref = st.solve(st.build_driver(), dict(pr, depth=np.zeros(300, np.float32), bl=np.float32(stereo_synth.BL)))
    for k in gen.OUTPUT_KEYS:
        np.testing.assert_array_equal(ref[k], g[f"kp300_m0_{k}"], err_msg=k)


def test_header_and_python_mirror_expose_the_marker_entries():
    hdr = open(os.path.join(ROOT, "include", "ucoslam_hip.h")).read()
    for sym in ("uh_pnp_solve_markers", "uh_pnp_solve_markers_dev", "uh_track_pose_markers"):
        assert re.search(r"\bint\s+" + sym + r"\s*\(", hdr), sym
    assert re.search(r"#define\s+UH_PNP_MAX_MARKERS\s+32\b", hdr) and "typedef struct uh_pnp_markers" in hdr
    import inspect

    from ucoslam_cv3_amd import pnp, projmatch

    assert "markers" in inspect.signature(pnp.PnPSolver.solvePnp).parameters
    assert "markers" in inspect.signature(projmatch.ProjectionMatcher.trackPoseMarkers).parameters
    assert pnp.MAX_MARKERS == 32
    assert [f[0] for f in pnp._Markers._fields_] == ["n", "pose_g2m", "size", "und_corners"]


# ------------------------------------------------------------------------------------------------ GPU
def _solver(ctx):
    from ucoslam_cv3_amd.pnp import PnPSolver

    return PnPSolver(ctx)


def _solve(sol, pr, **kw):
    return sol.solvePnp(pr["pose"], pr["intr"], pr["p3d"], pr["kp"], pr["invsig"], pr["weight"], depth=pr["depth"], bl=pr["bl"], **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_hip_markers_match_real_g2o(hip_ctx, name):
    g = _golden()
    pr = _problem(name)
    got = _solve(_solver(hip_ctx), pr, markers=pr["markers"])
    print(name, "iters", got["iters"].tolist(), g[f"{name}_iters"].tolist(), "ngood", got["ngood"], int(g[f"{name}_ngood"]), "state diff",
          np.abs(got["state"] - g[f"{name}_state"]).max(), "pose diff", np.abs(got["pose"] - g[f"{name}_pose"]).max())
    assert got["iters"].tolist() == g[f"{name}_iters"].tolist()
    assert got["ngood"] == int(g[f"{name}_ngood"])
    np.testing.assert_array_equal(got["bad"], g[f"{name}_bad"])
    assert np.abs(got["state"] - g[f"{name}_state"]).max() < POSE_TOL
    assert np.abs(got["pose"] - g[f"{name}_pose"]).max() < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["kp300_m2", "kp3001_m3", "m2_close"])
def test_hip_markers_dev_form_equals_host_form(hip_ctx, name):
    import torch

    from ucoslam_cv3_amd._lib import check, lib
    from ucoslam_cv3_amd.pnp import _Markers

    pr = _problem(name)
    sol = _solver(hip_ctx)
    host = _solve(sol, pr, markers=pr["markers"])
    n = len(pr["invsig"])
    dev = {k: torch.from_numpy(np.ascontiguousarray(pr[k], np.float32)).cuda() for k in marker_synth.INPUT_KEYS}
    mk = {k: torch.from_numpy(np.ascontiguousarray(pr["markers"][k], np.float32)).cuda() for k in marker_synth.MARKER_KEYS}
    work = torch.empty(max(n, 1) * 36, dtype=torch.uint8, device="cuda")
    pose_out = torch.zeros(16, dtype=torch.float32, device="cuda")
    bad = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
    res = torch.zeros(5, dtype=torch.int32, device="cuda")
    state = torch.zeros(7, dtype=torch.float64, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    ms = _Markers(len(pr["markers"]["size"]), ptr(mk["pose_g2m"]), ptr(mk["size"]), ptr(mk["und_corners"]))
    torch.cuda.synchronize()
    check(lib().uh_pnp_solve_markers_dev(sol._h, ptr(dev["pose"]), ptr(dev["intr"]), n, ptr(dev["p3d"]), ptr(dev["kp"]), ptr(dev["invsig"]),
                                         ptr(dev["weight"]), None, 0.0, C.byref(ms), ptr(work), ptr(pose_out), ptr(bad), ptr(res), ptr(state)))
    hip_ctx.synchronize()
    r = res.cpu().numpy()
    assert int(r[0]) == host["ngood"] and r[1:].tolist() == host["iters"].tolist()
    np.testing.assert_array_equal(bad.cpu().numpy()[:n], host["bad"])
    np.testing.assert_array_equal(state.cpu().numpy(), host["state"])
    np.testing.assert_array_equal(pose_out.cpu().numpy(), host["pose"])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [800, 3001])
@pytest.mark.parametrize("with_depth", [False, True])
def test_hip_no_markers_is_the_marker_free_solve_bit_for_bit(hip_ctx, n, with_depth):
    pr = stereo_synth.stereo_pnp_problem(n, seed=n) if with_depth else dict(synth.pnp_problem(n, seed=n), depth=None, bl=0.0)
    sol = _solver(hip_ctx)
    base = _solve(sol, pr)
    empty = dict(pose_g2m=np.zeros((0, 16), np.float32), size=np.zeros(0, np.float32), und_corners=np.zeros((0, 8), np.float32))
    from ucoslam_cv3_amd._lib import lib, np_ptr

    a = {k: np.ascontiguousarray(pr[k], np.float32) for k in marker_synth.INPUT_KEYS}
    d = None if pr["depth"] is None else np.ascontiguousarray(pr["depth"], np.float32)
    out = dict(pose=np.zeros(16, np.float32), bad=np.zeros(n, np.uint8), iters=np.zeros(4, np.int32), state=np.zeros(7))
    rc = lib().uh_pnp_solve_markers(sol._h, np_ptr(a["pose"]), np_ptr(a["intr"]), n, np_ptr(a["p3d"]), np_ptr(a["kp"]), np_ptr(a["invsig"]), np_ptr(a["weight"]),
                                    None if d is None else np_ptr(d), float(pr["bl"]), None, np_ptr(out["pose"]), np_ptr(out["bad"]), np_ptr(out["iters"]),
                                    np_ptr(out["state"]))
    for got, ngood in ((out, rc), (_solve(sol, pr, markers=empty), None)):
        for k in ("pose", "bad", "iters", "state"):
            np.testing.assert_array_equal(got[k], base[k], err_msg=k)
        assert (got["ngood"] if ngood is None else ngood) == base["ngood"]


@pytest.mark.gpu
def test_hip_markers_refuse_bad_arguments(hip_ctx):
    from ucoslam_cv3_amd._lib import lib, np_ptr
    from ucoslam_cv3_amd.pnp import _Markers

    pr = _problem("kp300_m2")
    sol = _solver(hip_ctx)
    a = {k: np.ascontiguousarray(pr[k], np.float32) for k in marker_synth.INPUT_KEYS}
    m = {k: np.ascontiguousarray(pr["markers"][k], np.float32) for k in marker_synth.MARKER_KEYS}
    n = len(a["invsig"])
    pose, bad, it, st = np.zeros(16, np.float32), np.zeros(n, np.uint8), np.zeros(4, np.int32), np.zeros(7)
    L = lib()

    def call(ms, n_=n, drop=()):
        args = [sol._h, np_ptr(a["pose"]), np_ptr(a["intr"]), n_, np_ptr(a["p3d"]), np_ptr(a["kp"]), np_ptr(a["invsig"]), np_ptr(a["weight"]), None,
                C.c_float(0.0), C.byref(ms) if ms is not None else None, np_ptr(pose), np_ptr(bad), np_ptr(it), np_ptr(st)]
        for i in drop:
            args[i] = None
        return L.uh_pnp_solve_markers(*args)

    ok = _Markers(2, np_ptr(m["pose_g2m"]), np_ptr(m["size"]), np_ptr(m["und_corners"]))
    assert call(ok) >= 0   # the complete call succeeds
    for i in (0, 1, 2, 4, 5, 6, 7, 11, 12):   # NULL handle, pose, intrinsics, match arrays, outputs
        assert call(ok, drop=(i,)) < 0, i
    for field in ("pose_g2m", "size", "und_corners"):   # each NULL marker array
        bad_m = _Markers(2, np_ptr(m["pose_g2m"]), np_ptr(m["size"]), np_ptr(m["und_corners"]))
        setattr(bad_m, field, None)
        assert call(bad_m) < 0, field
    big = dict(pose_g2m=np.tile(m["pose_g2m"][:1], (33, 1)), size=np.full(33, 0.2, np.float32), und_corners=np.tile(m["und_corners"][:1], (33, 1)))
    assert call(_Markers(33, np_ptr(big["pose_g2m"]), np_ptr(big["size"]), np_ptr(big["und_corners"]))) < 0
    assert call(_Markers(32, np_ptr(big["pose_g2m"]), np_ptr(big["size"]), np_ptr(big["und_corners"]))) >= 0   # the limit itself is served
    assert call(_Markers(-1, np_ptr(m["pose_g2m"]), np_ptr(m["size"]), np_ptr(m["und_corners"]))) < 0
    for v in (0.0, -0.1, np.nan, np.inf):
        sz = np.array([0.2, v], np.float32)
        assert call(_Markers(2, np_ptr(m["pose_g2m"]), np_ptr(sz), np_ptr(m["und_corners"]))) < 0, v
    # no matches: without markers the pose comes back as it went in, return value 0; with markers the match arrays may be NULL
    pose[:] = 0
    it[:] = 7
    assert call(_Markers(0, None, None, None), n_=0, drop=(4, 5, 6, 7, 12)) == 0
    np.testing.assert_array_equal(pose, a["pose"])
    assert it.tolist() == [0, 0, 0, 0]
    assert call(None, n_=0, drop=(4, 5, 6, 7, 12)) == 0
    assert call(ok, n_=0, drop=(4, 5, 6, 7, 12)) == 0 and it.tolist()[0] >= 1
    # device form: the same limits before anything is launched
    assert L.uh_pnp_solve_markers_dev(sol._h, np_ptr(a["pose"]), np_ptr(a["intr"]), 0, None, None, None, None, None, C.c_float(0.0),
                                      C.byref(_Markers(33, np_ptr(big["pose_g2m"]), np_ptr(big["size"]), np_ptr(big["und_corners"]))), None, np_ptr(pose), None,
                                      np_ptr(it), None) < 0
    assert L.uh_pnp_solve_markers_dev(sol._h, np_ptr(a["pose"]), np_ptr(a["intr"]), 0, None, None, None, None, None, C.c_float(0.0),
                                      C.byref(_Markers(2, None, np_ptr(m["size"]), np_ptr(m["und_corners"]))), None, np_ptr(pose), None, np_ptr(it), None) < 0
