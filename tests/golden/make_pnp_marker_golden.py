"""Generates tests/golden/pnp_marker_golden.npz: pose-only PnP with keypoint matches and squared planar markers on the REAL reference g2o.

The driver tests/golden/pnp_marker_ref.cpp is compiled against the g2o objects that `make -C oracle ref` leaves in oracle/_ref/obj/
(the reference tree's headers are needed as well) into oracle/_ref/libpnp_marker_ref.so.  Inputs: tests/marker_synth.py (CASES);
the fixture keeps a digest of every case's inputs and the reference's outputs (pose, se3 state, bad flags, inliers, iterations).

The jitter screen: the marker edge rounds its projections to float and g2o differentiates it numerically, so the reference itself is
discontinuous — a relative nudge of 1e-12 on the projected corners changes the outcome of a few percent of random problems.  A case is
admitted only if the driver's eight jitter patterns (camera-frame corner coordinates times 1 +- 1e-11, 1 +- 0.7e-11 for z) all give the
same iterations, the same bad flags and a state within SCREEN_TOL of the unjittered one; otherwise generate() fails and names the seed
to replace in marker_synth.CASES.
Build container only:  python tests/golden/make_pnp_marker_golden.py"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, TESTS)
import marker_synth  # noqa: E402
import oracle_lib  # noqa: E402

ORACLE = os.path.join(ROOT, "oracle")
OBJ = os.path.join(ORACLE, "_ref", "obj")
LIB = os.path.join(ORACLE, "_ref", "libpnp_marker_ref.so")
SRC = os.path.join(HERE, "pnp_marker_ref.cpp")
GOLDEN = os.path.join(HERE, "pnp_marker_golden.npz")
OUTPUT_KEYS = ("pose", "state", "bad", "ngood", "iters")
JITTERS = range(1, 9)
SCREEN_TOL = 1e-9


def reference_tree():
    """The reference tree the oracle Makefile builds from (REF ?= ... in oracle/Makefile, or $REF)."""
    ref = os.environ.get("REF")
    if not ref:
        m = re.search(r"^REF\s*\?=\s*(\S+)", open(os.path.join(ORACLE, "Makefile")).read(), re.M)
        ref = m.group(1) if m else ""
    return ref


def driver_available():
    """Why the driver cannot be built here, or None when it can."""
    if not os.path.exists(os.path.join(OBJ, ".g2o_done")):
        return "oracle/_ref/obj is not built (make -C oracle ref)"
    ref = reference_tree()
    if not os.path.exists(os.path.join(ref, "3rdparty", "g2o", "g2o", "core", "base_binary_edge.h")):
        return "the reference tree's g2o headers are not present"
    return None


def build_driver():
    """Compile the driver with the oracle Makefile's reference flags; returns the loaded library."""
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < os.path.getmtime(SRC):
        ref = reference_tree()
        g2o = os.path.join(ref, "3rdparty", "g2o")
        objs = sorted(os.path.join(OBJ, f) for f in os.listdir(OBJ) if f.endswith(".o"))
        cmd = ["g++", "-std=c++11", "-O3", "-mavx", "-msse3", "-mpopcnt", "-fPIC", "-w", "-DNDEBUG", f"-I{g2o}",
               f"-I{os.path.join(ref, '3rdparty', 'eigen3', 'eigen3')}", f"-I{os.path.join(g2o, 'g2o', 'stuff')}", "-shared", "-o", LIB, SRC,
               *objs, "-lpthread"]
        subprocess.check_call(cmd)
    L = C.CDLL(LIB)
    L.pnp_marker_ref_solve.restype = C.c_int
    L.pnp_marker_ref_solve.argtypes = [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 5 + [C.c_float, C.c_int] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 4
    return L


def solve(L, pr, jitter=0):
    P = oracle_lib.P
    a = {k: np.ascontiguousarray(pr[k], np.float32) for k in marker_synth.INPUT_KEYS}
    mk = {k: np.ascontiguousarray(pr["markers"][k], np.float32) for k in marker_synth.MARKER_KEYS}
    depth = None if pr["depth"] is None else np.ascontiguousarray(pr["depth"], np.float32)
    n, nm = len(a["invsig"]), len(mk["size"])
    pose = np.zeros(16, np.float32)
    bad = np.zeros(max(n, 1), np.uint8)
    iters = np.zeros(4, np.int32)
    state = np.zeros(7, np.float64)
    ngood = L.pnp_marker_ref_solve(P(a["pose"]), P(a["intr"]), n, P(a["p3d"]), P(a["kp"]), P(a["invsig"]), P(a["weight"]),
                                   None if depth is None else P(depth), float(pr["bl"]), nm, P(mk["pose_g2m"]), P(mk["size"]), P(mk["und_corners"]),
                                   int(jitter), P(pose), P(bad), P(iters), P(state))
    return dict(pose=pose, state=state, bad=bad[:n], ngood=np.int32(ngood), iters=iters)


def input_digest(pr):
    arrays = [np.ascontiguousarray(pr[k], np.float32) for k in marker_synth.INPUT_KEYS]
    arrays += [np.ascontiguousarray(pr["markers"][k], np.float32) for k in marker_synth.MARKER_KEYS]
    if pr["depth"] is not None:
        arrays.append(np.ascontiguousarray(pr["depth"], np.float32))
    return oracle_lib.digest(*arrays, np.float32(pr["bl"]))


def screen(L, pr, base):
    """None when all eight jittered runs agree with the unjittered one, else what differs."""
    for j in JITTERS:
        out = solve(L, pr, j)
        if out["iters"].tolist() != base["iters"].tolist():
            return f"jitter {j}: iterations {out['iters'].tolist()} != {base['iters'].tolist()}"
        if not np.array_equal(out["bad"], base["bad"]):
            return f"jitter {j}: {int((out['bad'] != base['bad']).sum())} bad flags differ"
        d = float(np.abs(out["state"] - base["state"]).max())
        if not d <= SCREEN_TOL:
            return f"jitter {j}: state moves by {d:.3g} > {SCREEN_TOL:g}"
    return None


def generate():
    L = build_driver()
    save = {}
    for name, kw in marker_synth.CASES.items():
        pr = marker_synth.marker_pnp_problem(**kw)
        out = solve(L, pr)
        why = screen(L, pr, out)
        assert why is None, f"case {name} (seed {kw['seed']}) does not pass the jitter screen — replace its seed in marker_synth.CASES: {why}"
        assert np.isfinite(out["state"]).all() and np.isfinite(out["pose"]).all(), name
        save[f"{name}_in_digest"] = input_digest(pr)
        for k in OUTPUT_KEYS:
            save[f"{name}_{k}"] = out[k]
        print(name, "n", len(pr["invsig"]), "markers", len(pr["markers"]["size"]), "ngood", int(out["ngood"]), "iters", out["iters"].tolist())
    return save


if __name__ == "__main__":
    why = driver_available()
    assert why is None, why
    np.savez_compressed(GOLDEN, **generate())
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
