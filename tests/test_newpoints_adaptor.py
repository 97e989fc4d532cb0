"""The new-map-point adaptors (include/ucoslam_hip/adaptors.hpp: Triangulate, NewPointCreator) on toy frames through
tests/host_helpers/newpoints_adaptor.cpp: the Se3 helpers on the host; on a GPU one 3-neighbour scene, whose result equals the Python
mirror's on the same frames bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import newpoints_oracle as O
import newpoints_synth as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ucoslam-cv3_amd", "libucoslam_hip.so")


def _build(tmp_path):
    exe = str(tmp_path / "newpoints_adaptor")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "host_helpers", "newpoints_adaptor.cpp"),
                           "-L", os.path.dirname(LIB), "-lucoslam_hip", f"-Wl,-rpath,{os.path.dirname(LIB)}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_newpoints_adaptor_host_helpers(tmp_path):
    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "newpoints host ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_newpoints_adaptor_equals_python_mirror(hip_ctx, tmp_path):
    from ucoslam_cv3_amd.newpoints import NewPoints

    dump = str(tmp_path / "adaptor.bin")
    out = subprocess.run([_build(tmp_path), dump], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "newpoints adaptor ok" in out.stdout, out.stdout + out.stderr
    raw = open(dump, "rb").read()
    off = 0

    def take(dtype, count=1):
        nonlocal off
        a = np.frombuffer(raw, dtype, count, off).copy()
        off += a.nbytes
        return a

    def frame():
        idx, n = take(np.int32, 2).tolist()
        return idx, take(np.float32, 16).reshape(4, 4), take(np.float32, 2 * n).reshape(n, 2), take(np.int32, n)

    sf = take(np.float32, int(take(np.int32)[0]))
    idx_new, pose, pt, octave = frame()
    kf = S.make_new_kf(pose, pt, octave, scale_factors=sf)
    pairs, ids = [], []
    for j in range(3):
        idx, p2, pt2, oct2 = frame()
        RT = take(np.float32, 16).reshape(4, 4)
        m = take(O.DMATCH_DTYPE, int(take(np.int32)[0]))
        pair = S.make_pair(kf, p2, pt2, oct2, [], scale_factors=sf)
        assert O.ulp_diff(pair["RT"], RT).max() <= 1      # the adaptor's RT against numpy's float64 product of the same factors
        pair["RT"], pair["matches"] = RT, m
        pairs.append(pair)
        ids.append(idx)
    got = NewPoints(hip_ctx).run(kf, pairs, ratio_factor=float(np.float32(1.5) * np.float32(1.2)))
    n_new = int(take(np.int32)[0])
    assert n_new == got["n_new"] and 10 < n_new < 45 and (got["status"] != 0).any()
    for i in range(n_new):
        assert int(take(np.int32)[0]) == got["kp_idx"][i]
        assert take(np.float32, 3).tobytes() == got["xyz_global"][i].tobytes()
        assert take(np.float32).tobytes() == got["distance"][i:i + 1].tobytes()
        n_obs = int(take(np.int32)[0])
        fk = take(np.int32, 2 * n_obs).reshape(n_obs, 2)
        a, b = got["obs_ptr"][i], got["obs_ptr"][i + 1]
        assert n_obs == b - a
        assert fk[:, 0].tolist() == [idx_new if p < 0 else ids[p] for p in got["obs_pair"][a:b]]
        assert fk[:, 1].tolist() == got["obs_kpt"][a:b].tolist()
    n0 = len(pairs[0]["matches"])
    tri = take(np.float32, 3 * n0).reshape(n0, 3)
    assert off == len(raw)
    assert tri.tobytes() == got["xyz_cam"][:n0].tobytes() and np.isnan(tri).any() and np.isfinite(tri).any()
