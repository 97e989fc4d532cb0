"""examples/relocalize_one_call.cpp: the scene of examples/relocalize.cpp through the chain of single calls and through
ucoslam_hip::Relocalizer::relocalize (include/ucoslam_hip/adaptors.hpp, ONE uh_relocalize_pose) from a C++ host; the program compares every
stage, list, flag, count and pose of the two routes itself and ends non-zero on any difference.  Its winner line is the one the existing
example prints."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run(tmp_path, name):
    lib_dir = os.path.join(ROOT, "ucoslam-cv3_amd")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", exe, os.path.join(ROOT, "examples", name + ".cpp"), "-L", lib_dir, "-lucoslam_hip",
                           f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    return subprocess.run([exe], capture_output=True, text=True, timeout=120)


def test_one_call_example_equals_the_chain_of_single_calls(tmp_path):
    one = _build_and_run(tmp_path, "relocalize_one_call")
    assert one.returncode == 0 and "DIFFERENT" not in one.stdout, one.stdout + one.stderr
    ref = _build_and_run(tmp_path, "relocalize")
    assert ref.returncode == 0, ref.stdout + ref.stderr
    winner = [l for l in ref.stdout.splitlines() if l.startswith("relocalised on candidate")]
    assert len(winner) == 1 and winner[0] in one.stdout.splitlines(), (winner, one.stdout)
