"""The stereo / RGB-D adaptors (include/ucoslam_hip/adaptors.hpp: FrameExtractor::processStereo / process_rgbd) on a toy Frame through
tests/host_helpers/stereo_adaptor.cpp: the host form through the C ABI on a scene with a closed-form depth; on a GPU both adaptors on a
procedural image pair, whose frames equal the Python mirror's on the same images byte for byte, and the oracle's depth."""
import os
import subprocess

import numpy as np
import pytest

import stereo_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ucoslam-cv3_amd", "libucoslam_hip.so")
UND_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])


def _build(tmp_path):
    exe = str(tmp_path / "stereo_adaptor")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "host_helpers", "stereo_adaptor.cpp"),
                           "-L", os.path.dirname(LIB), "-lucoslam_hip", f"-Wl,-rpath,{os.path.dirname(LIB)}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_stereo_adaptor_host_form(tmp_path):
    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "stereo host ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_stereo_frame_example_tracks_with_the_depths_it_extracted(hip_ctx, tmp_path):
    """examples/stereo_frame.cpp: uh_orb_extract_stereo -> uh_projmatch_set_frame_dev -> uh_track_pose_stereo from a C++ host, on a map made of
    the frame's own depths: tracked, and back at the pose the map was made from (the program exits non-zero otherwise)."""
    import json

    exe = str(tmp_path / "stereo_frame")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-o", exe, os.path.join(ROOT, "examples", "stereo_frame.cpp"),
                           "-L", os.path.dirname(LIB), "-lucoslam_hip", f"-Wl,-rpath,{os.path.dirname(LIB)}", "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, "3"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])
    print(r)
    assert r["tracked"] == 1 and r["with_depth"] > 0.5 * r["keypoints"] and r["inliers2"] > 0.5 * r["map_points"] and r["translation_error_m"] < 0.02


@pytest.mark.gpu
def test_stereo_adaptor_equals_python_mirror(hip_ctx, tmp_path):
    from ucoslam_cv3_amd.orb import Camera, FeatParams, ORBextractor
    from ucoslam_cv3_amd.stereo import extract_rgbd, extract_stereo, set_stereo

    dump = str(tmp_path / "adaptor.bin")
    out = subprocess.run([_build(tmp_path), dump], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "stereo adaptor ok" in out.stdout, out.stdout + out.stderr
    raw = open(dump, "rb").read()
    off = 0

    def take(dtype, count=1):
        nonlocal off
        a = np.frombuffer(raw, dtype, count, off).copy()
        off += a.nbytes
        return a

    def frame():
        n = int(take(np.int32)[0])
        return dict(kpts=take(np.float32, 2 * n).reshape(n, 2), und=take(UND_DTYPE, n), desc=take(np.uint8, 32 * n).reshape(n, 32), depth=take(np.float32, n),
                    fseq=int(take(np.uint32)[0]))

    w, h = take(np.int32, 2).tolist()
    left, right, D = take(np.uint8, w * h).reshape(h, w), take(np.uint8, w * h).reshape(h, w), take(np.uint16, w * h).reshape(h, w)
    fs, fd = frame(), frame()
    assert off == len(raw) and fs["fseq"] == 41 and fd["fseq"] == 42
    ext = ORBextractor(hip_ctx)
    ext.detectAndCompute(np.zeros((0, 0), np.uint8), None, FeatParams(800, 5, 1.2))
    ext.setCamera(Camera(517.3, 516.5, 158.6, 99.3, ()))
    set_stereo(ext, 0.11, 50.0)
    for f, r in ((fs, extract_stereo(ext, left, right, want_right=True)), (fd, extract_rgbd(ext, left, D, np.float32(1.0 / 5000.0)))):
        n = len(r["kps"])
        assert n == len(f["und"]) and n > 100
        assert f["kpts"].tobytes() == np.stack([r["kps"]["x"], r["kps"]["y"]], 1).tobytes()
        assert f["und"]["x"].tobytes() == r["und_xy"][:, 0].tobytes() and f["und"]["y"].tobytes() == r["und_xy"][:, 1].tobytes()
        for k in ("size", "angle", "response", "octave", "class_id"):
            assert f["und"][k].tobytes() == r["kps"][k].tobytes()
        assert f["desc"].tobytes() == r["desc"].tobytes() and f["depth"].tobytes() == r["depth"].tobytes()
    rs = extract_stereo(ext, left, right, want_right=True)
    want, _ = O.stereo_depth(left, right, fs["und"], fs["desc"], rs["right_kps"], rs["right_desc"], 0.11, 517.3, 50.0)
    assert fs["depth"].tobytes() == want.tobytes() and float((want > 0).mean()) > 0.3
    assert fd["depth"].tobytes() == O.rgbd_depth(rs["kps"], D, np.float32(1.0 / 5000.0)).tobytes() and (fd["depth"] == 0).any() and (fd["depth"] > 0).any()
