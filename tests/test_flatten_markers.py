"""flatten_for_ba_markers (include/ucoslam_hip/flatten_ba.hpp): the marker part of GlobalOptimizerG2O::setParams
(globaloptimizer_g2o.cpp:156-171 the join rule, :281-299 the weights, :320-352 the edge order, :355-398 the planar constraint, refused)
on a toy map.  The C++ program (tests/host_helpers/flatten_markers_test.cpp) checks the structure against hand-derived sets and prints
the flattened problem; the weights are checked here against a straight restatement of :281-299.  Pure host C++, no GPU."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reference_weight(kpw, n_markers, markers_opt_weight, min_markers_for_max_weight):
    """globaloptimizer_g2o.cpp:285-297 for one frame: kpw a double, markersOptWeight a float, minMarkersForMaxWeight an int."""
    weight_per_error = 1.0
    if kpw > 40 and n_markers > 0:
        marker_perct = float(np.float32(markers_opt_weight)) * min(1.0, float(n_markers) / min_markers_for_max_weight)
        total_w = marker_perct * kpw
        weight_per_error = total_w / float(n_markers * 8)
    return weight_per_error


def test_flatten_for_ba_markers_rules_on_a_toy_map(tmp_path):
    exe = str(tmp_path / "flatten_markers_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "host_helpers", "flatten_markers_test.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "flatten markers ok" in out.stdout, out.stdout + out.stderr
    rec = [l.split() for l in out.stdout.splitlines()]
    n_markers = {int(r[1]): int(r[3]) for r in rec if r[0] == "frame"}
    assert n_markers == {0: 1, 1: 3, 2: 1, 3: 1}            # frame 1 counts its marker without a valid pose
    # kpw (:248, :271): per edge of the frame, in edge order, the float product 2 * f or 3 * f added to a double
    kpw = {k: 0.0 for k in n_markers}
    n_stereo = 0
    for r in rec:
        if r[0] == "obs":
            k, inv, depth = int(r[1]), float(r[2]), float(r[3])
            assert inv == float(np.float32(inv))
            kpw[k] += float(np.float32(3 if depth > 0 else 2) * np.float32(inv))
            n_stereo += depth > 0
    assert n_stereo == 6 and kpw[0] > 40 and kpw[1] > 40 and 0 < kpw[2] <= 40 and kpw[3] == 0
    for tag, mow, mmw in (("edge", 0.5, 5), ("edge2", 0.25, 2)):
        edges = [(int(r[1]), int(r[2]), float(r[3])) for r in rec if r[0] == tag]
        assert [(m, k) for m, k, _ in edges] == [(0, 1), (0, 2), (1, 0), (1, 1), (1, 3)]
        for m, k, w in edges:
            assert w == _reference_weight(kpw[k], n_markers[k], mow, mmw), (tag, m, k)
        assert edges[1][2] == 1.0 and edges[4][2] == 1.0     # kpw <= 40, and a frame that joined through the marker
        assert edges[0][2] != 1.0 and edges[2][2] != 1.0 and edges[0][2] == edges[3][2]
