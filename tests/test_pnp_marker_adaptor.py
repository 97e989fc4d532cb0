"""The marker overload of the C++ adaptor PnPSolver::solvePnp (include/ucoslam_hip/adaptors.hpp) compiles with g++ against the library,
fails loudly without a GPU and solves a small problem with markers, and a marker-only one, on a GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ucoslam-cv3_amd", "libucoslam_hip.so")


def _build(tmp_path):
    exe = str(tmp_path / "pnp_marker_adaptor")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "host_helpers", "pnp_marker_adaptor.cpp"),
                           "-L", os.path.dirname(LIB), "-lucoslam_hip", f"-Wl,-rpath,{os.path.dirname(LIB)}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_marker_adaptor_compiles_and_fails_loudly_without_gpu(tmp_path):
    import torch

    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    if not torch.cuda.is_available():
        assert "no device" in out.stdout


@pytest.mark.gpu
def test_marker_adaptor_solves_on_gpu(tmp_path):
    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "markers ok: 60 inliers" in out.stdout, out.stdout
