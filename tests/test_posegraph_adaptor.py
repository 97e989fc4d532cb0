"""The loop-closure adaptor (include/ucoslam_hip/adaptors.hpp: loopClosurePathOptimization with the reference's argument list) on a toy
map through tests/host_helpers/posegraph_adaptor.cpp: the flattening (std::map key order, weights under CovisGraph::join's key, write-back,
the throw above the cap) on the host; on a GPU the whole call equals the Python route on the same flattened arrays bit for bit."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ucoslam-cv3_amd", "libucoslam_hip.so")


def _build(tmp_path):
    exe = str(tmp_path / "posegraph_adaptor")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "host_helpers", "posegraph_adaptor.cpp"),
                           "-L", os.path.dirname(LIB), "-lucoslam_hip", f"-Wl,-rpath,{os.path.dirname(LIB)}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_posegraph_adaptor_flattens_a_toy_map(tmp_path):
    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "posegraph flatten ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_posegraph_adaptor_equals_python_route(hip_ctx, tmp_path):
    from ucoslam_cv3_amd.posegraph import PoseGraph

    dump = str(tmp_path / "adaptor.bin")
    out = subprocess.run([_build(tmp_path), dump], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "posegraph adaptor ok" in out.stdout, out.stdout + out.stderr
    raw = open(dump, "rb").read()
    n, E, idx_new, idx_old = np.frombuffer(raw, np.int32, 4).tolist()
    assert (n, E, idx_new, idx_old) == (5, 4, 2, 3)
    off = 16

    def take(dtype, count):
        nonlocal off
        a = np.frombuffer(raw, dtype, count, off).copy()
        off += a.nbytes
        return a

    poses, ei, ej, w, expected, cpp = take(np.float32, 16 * n).reshape(n, 16), take(np.int32, E), take(np.int32, E), take(np.float32, E), take(np.float32, 16), take(np.float32, 16 * n).reshape(n, 16)
    assert off == len(raw)
    pg = PoseGraph(hip_ctx)
    got = pg.optimize(poses, ei, ej, w, idx_new, idx_old, expected, True)
    np.testing.assert_array_equal(cpp, got["poses"])
    assert got["iterations"] >= 2 and got["chi2_after"] < 0.5 * got["chi2_before"]
    np.testing.assert_array_equal(cpp[0], poses[0])                      # the pose without edges: identity rotation, exact round trip
    np.testing.assert_array_equal(cpp[idx_old], poses[idx_old])          # the fixed pose
    assert np.abs(cpp[[1, 4]] - poses[[1, 4]]).max() > 1e-3              # the free ones moved
    pg.close()
