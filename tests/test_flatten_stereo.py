"""flatten_for_ba_stereo (include/ucoslam_hip/flatten_ba.hpp) on a toy map with depths: edge order, depth / baseline placement, a
single-observer stereo point taken (globaloptimizer_g2o.cpp:142), a single-observer non-stereo point rejected, flatten_for_ba still
refusing the same map, and the sizes / offsets of the new ABI structs.  Pure host C++, no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flatten_for_ba_stereo_on_a_toy_map(tmp_path):
    exe = str(tmp_path / "flatten_stereo_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "host_helpers", "flatten_stereo_test.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "flatten stereo ok" in out.stdout, out.stdout + out.stderr
