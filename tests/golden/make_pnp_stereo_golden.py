"""Generates tests/golden/pnp_stereo_golden.npz: pose-only PnP with stereo / RGB-D observations on the REAL reference g2o.

The driver tests/golden/pnp_stereo_ref.cpp is compiled against the g2o objects that `make -C oracle ref` leaves in oracle/_ref/obj/
(the reference tree's headers are needed as well) into oracle/_ref/libpnp_stereo_ref.so.  Inputs: tests/stereo_synth.py (CASES);
the fixture keeps a digest of every case's inputs and the reference's outputs (pose, se3 state, bad flags, inliers, iterations).
Build container only:  python tests/golden/make_pnp_stereo_golden.py"""
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
import oracle_lib  # noqa: E402
import stereo_synth  # noqa: E402

ORACLE = os.path.join(ROOT, "oracle")
OBJ = os.path.join(ORACLE, "_ref", "obj")
LIB = os.path.join(ORACLE, "_ref", "libpnp_stereo_ref.so")
SRC = os.path.join(HERE, "pnp_stereo_ref.cpp")
GOLDEN = os.path.join(HERE, "pnp_stereo_golden.npz")
OUTPUT_KEYS = ("pose", "state", "bad", "ngood", "iters")


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
    if not os.path.exists(os.path.join(ref, "3rdparty", "g2o", "g2o", "core", "base_unary_edge.h")):
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
    L.pnp_stereo_ref_solve.restype = C.c_int
    L.pnp_stereo_ref_solve.argtypes = [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 5 + [C.c_float] + [C.c_void_p] * 4
    return L


def solve(L, pr):
    P = oracle_lib.P
    a = {k: np.ascontiguousarray(pr[k], np.float32) for k in stereo_synth.INPUT_KEYS}
    n = len(a["invsig"])
    pose = np.zeros(16, np.float32)
    bad = np.zeros(max(n, 1), np.uint8)
    iters = np.zeros(4, np.int32)
    state = np.zeros(7, np.float64)
    ngood = L.pnp_stereo_ref_solve(P(a["pose"]), P(a["intr"]), n, P(a["p3d"]), P(a["kp"]), P(a["invsig"]), P(a["weight"]), P(a["depth"]),
                                   float(pr["bl"]), P(pose), P(bad), P(iters), P(state))
    return dict(pose=pose, state=state, bad=bad[:n], ngood=np.int32(ngood), iters=iters)


def input_digest(pr):
    return oracle_lib.digest(*[np.ascontiguousarray(pr[k], np.float32) for k in stereo_synth.INPUT_KEYS], np.float32(pr["bl"]))


def generate():
    L = build_driver()
    save = {}
    for name, kw in stereo_synth.CASES.items():
        pr = stereo_synth.stereo_pnp_problem(**kw)
        out = solve(L, pr)
        save[f"{name}_in_digest"] = input_digest(pr)
        for k in OUTPUT_KEYS:
            save[f"{name}_{k}"] = out[k]
        print(name, "n", len(pr["invsig"]), "stereo", int((pr["depth"] > 0).sum()), "ngood", int(out["ngood"]), "iters", out["iters"].tolist())
    return save


if __name__ == "__main__":
    why = driver_available()
    assert why is None, why
    np.savez_compressed(GOLDEN, **generate())
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
