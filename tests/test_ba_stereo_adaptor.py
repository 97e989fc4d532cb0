"""The stereo route of the C++ adaptor GlobalOptimizer (include/ucoslam_hip/adaptors.hpp): compiles with g++ against the library, fails
loudly without a GPU; on one, toy map -> flatten_for_ba_stereo -> staging block -> optimise -> apply_results equals the Python route
(uh_ba_set_problem_stereo on the same flattened arrays) bit for bit."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ucoslam-cv3_amd", "libucoslam_hip.so")


def _build(tmp_path):
    exe = str(tmp_path / "ba_stereo_adaptor")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "host_helpers", "ba_stereo_adaptor.cpp"),
                           "-L", os.path.dirname(LIB), "-lucoslam_hip", f"-Wl,-rpath,{os.path.dirname(LIB)}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_ba_stereo_adaptor_compiles_and_fails_loudly_without_gpu(tmp_path):
    import torch

    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    if not torch.cuda.is_available():
        assert "no device" in out.stdout


@pytest.mark.gpu
def test_ba_stereo_adaptor_equals_python_route(hip_ctx, tmp_path):
    from ucoslam_cv3_amd.ba import OBS_DTYPE, GlobalOptimizer, ParamSet

    dump = str(tmp_path / "adaptor.bin")
    out = subprocess.run([_build(tmp_path), dump], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ba stereo ok" in out.stdout, out.stdout + out.stderr
    raw = open(dump, "rb").read()
    K, P, E, nbad = np.frombuffer(raw, np.int32, 4).tolist()
    off = 16

    def take(dtype, n):
        nonlocal off
        a = np.frombuffer(raw, dtype, n, off).copy()
        off += a.nbytes
        return a

    pr = dict(poses=take(np.float32, 16 * K).reshape(K, 16), fixed=take(np.uint8, K), intr=take(np.float32, 4 * K).reshape(K, 4),
              points=take(np.float32, 3 * P).reshape(P, 3))
    obs = take(OBS_DTYPE, E)
    pr.update(obs_pt=np.ascontiguousarray(obs["point"]), obs_kf=np.ascontiguousarray(obs["frame"]),
              obs_uv=np.ascontiguousarray(np.stack([obs["u"], obs["v"]], 1)), obs_w=np.ascontiguousarray(obs["inv_sigma"]),
              obs_depth=take(np.float32, E), frame_bl=take(np.float32, K))
    cpp_poses, cpp_points = take(np.float32, 16 * K).reshape(K, 16), take(np.float32, 3 * P).reshape(P, 3)
    assert off == len(raw)
    opt = GlobalOptimizer.create(hip_ctx)
    opt.setParams(pr, ParamSet(nIters=5), stereo=True)
    assert opt.form() == "chain"
    opt.optimize()
    got = opt.getResults()
    np.testing.assert_array_equal(cpp_poses, got["poses"])
    np.testing.assert_array_equal(cpp_points, got["points"])
    assert nbad == int(got["bad"].sum())
    assert np.abs(got["poses"][1:] - pr["poses"][1:]).max() > 1e-4      # the free frames did move
