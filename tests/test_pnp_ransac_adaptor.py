"""The C++ adaptor PnPSolver::solvePnPRansac (include/ucoslam_hip/adaptors.hpp), single and batched overload, compiles with g++ against
stub views and the library, fails loudly without a GPU, and on one solves a planted scene beside a candidate of three matches and one of
wrong matches; its result equals the Python mirror's on the same arrays and the same rand() sequence bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ucoslam-cv3_amd", "libucoslam_hip.so")


def _build(tmp_path):
    exe = str(tmp_path / "pnp_ransac_adaptor")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "host_helpers", "pnp_ransac_adaptor.cpp"),
                           "-L", os.path.dirname(LIB), "-lucoslam_hip", f"-Wl,-rpath,{os.path.dirname(LIB)}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_ransac_adaptor_compiles_and_fails_loudly_without_gpu(tmp_path):
    import torch

    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    if not torch.cuda.is_available():
        assert "no device" in out.stdout


@pytest.mark.gpu
def test_ransac_adaptor_equals_python_mirror(hip_ctx, tmp_path):
    from ucoslam_cv3_amd import PnPRansac, ransac_samples

    dump = str(tmp_path / "adaptor.bin")
    out = subprocess.run([_build(tmp_path), dump], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ransac adaptor ok: 64 inliers" in out.stdout, out.stdout + out.stderr
    raw = open(dump, "rb").read()
    n, n_in = np.frombuffer(raw, np.int32, 2).tolist()
    rec = np.frombuffer(raw, np.float32, 8 * n, 8).reshape(n, 8)
    rt6 = np.frombuffer(raw, np.float32, 6, 8 + 32 * n)
    kept = np.frombuffer(raw, np.int32, n_in, 8 + 32 * n + 24)
    C.CDLL(None).srand(C.c_uint(4711))
    pr = dict(p3d=rec[:, 0:3], normal=rec[:, 3:6], kp=rec[:, 6:8], samples=ransac_samples(n, 50), rt6_in=np.array([0.01, 0.02, 0.03, 0, 0, 0], np.float32))
    got = PnPRansac(hip_ctx).solve([718.856, 718.856, 607.19, 185.22], [pr])[0]
    assert got["ok"] == 1 and got["inliers"].tolist() == kept.tolist() and got["rt6"].tobytes() == rt6.tobytes()
