"""The marker route of the C++ adaptor GlobalOptimizer (include/ucoslam_hip/adaptors.hpp): compiles with g++ against the library, fails
loudly without a GPU; on one, a toy map of mk_single's shape (4 keyframes, one fixed, ~120 landmarks, one marker seen by two free frames
and the fixed one) -> flatten_for_ba_markers -> uh_ba_set_problem_markers -> optimise -> apply_results / apply_marker_results equals the
Python route on the same flattened arrays bit for bit."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ucoslam-cv3_amd", "libucoslam_hip.so")


def _build(tmp_path):
    exe = str(tmp_path / "ba_marker_adaptor")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "host_helpers", "ba_marker_adaptor.cpp"),
                           "-L", os.path.dirname(LIB), "-lucoslam_hip", f"-Wl,-rpath,{os.path.dirname(LIB)}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_ba_marker_adaptor_compiles_and_fails_loudly_without_gpu(tmp_path):
    import torch

    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    if not torch.cuda.is_available():
        assert "no device" in out.stdout


@pytest.mark.gpu
def test_ba_marker_adaptor_equals_python_route(hip_ctx, tmp_path):
    from ucoslam_cv3_amd.ba import OBS_DTYPE, GlobalOptimizer, ParamSet

    dump = str(tmp_path / "adaptor.bin")
    out = subprocess.run([_build(tmp_path), dump], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ba marker ok" in out.stdout, out.stdout + out.stderr
    raw = open(dump, "rb").read()
    K, P, E, M, EM, nbad = np.frombuffer(raw, np.int32, 6).tolist()
    assert (K, M, EM) == (4, 1, 3)
    off = 24

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
    mk = dict(pose_g2m=take(np.float32, 16 * M).reshape(M, 16), size=take(np.float32, M), edge_marker=take(np.int32, EM), edge_frame=take(np.int32, EM),
              und_corners=take(np.float32, 8 * EM).reshape(EM, 8), edge_weight=take(np.float64, EM))
    cpp_poses, cpp_points, cpp_markers = take(np.float32, 16 * K).reshape(K, 16), take(np.float32, 3 * P).reshape(P, 3), take(np.float32, 16 * M).reshape(M, 16)
    assert off == len(raw)
    assert pr["fixed"].tolist() == [1, 0, 0, 0] and mk["edge_frame"].tolist() == [0, 1, 2] and (mk["edge_weight"] != 1.0).all()
    opt = GlobalOptimizer.create(hip_ctx)
    opt.setParams(pr, ParamSet(nIters=5), stereo=True, markers=mk)
    assert opt.form() == "wide"
    opt.optimize()
    got = opt.getResults()
    np.testing.assert_array_equal(cpp_poses, got["poses"])
    np.testing.assert_array_equal(cpp_points, got["points"])
    np.testing.assert_array_equal(cpp_markers, opt.getMarkerResults()["poses"])
    assert nbad == int(got["bad"].sum())
    assert np.abs(got["poses"][1:] - pr["poses"][1:]).max() > 1e-4      # the free frames did move
    assert np.abs(cpp_markers - mk["pose_g2m"]).max() > 1e-4            # ... and the marker
