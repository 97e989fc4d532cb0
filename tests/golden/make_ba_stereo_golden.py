"""Generates tests/golden/ba_stereo_golden.npz: bundle adjustment with stereo / RGB-D observations on the REAL reference g2o.

The driver tests/golden/ba_stereo_ref.cpp is compiled against the g2o objects that `make -C oracle ref` leaves in oracle/_ref/obj/
(the reference tree's headers are needed as well) into oracle/_ref/libba_stereo_ref.so.  Inputs: tests/stereo_ba_synth.py (CASES);
the fixture keeps a digest of every case's inputs and the reference's outputs (poses, points, se3 state, chi2, bad flags, iterations).

Three conditions are asserted on every case, so that the GPU tests compare without an escape clause (margins are printed):
  1. no edge's between-pass or final chi2 within 1e-6 (1 + limit) of its own limit (5.99 / 7.815), no camera-frame z of a depth test
     within 1e-9 of 0;
  2. the driver run again with every kp_ur moved by +-1e-9 px (in double, sign alternating with the edge index) gives the same
     iteration counts and bad flags and an se3 state within 1e-7 — rounding differences between two implementations act like a
     perturbation of ~1e-12 px, so a case that passes sits three orders inside the 1e-6 tolerance of the comparison;
     The same for the one difference between driver and product that is known in advance: the reference holds the two-row edges'
     limit and Huber width as floats (5.99f, (float)sqrt(5.99f)), the product's monocular defaults are the doubles 5.99 and sqrt(5.99)
     — 2.3e-7 apart on the limit, 4.6e-8 relative on the width, which reweights every pass-1 outlier of a mixed problem.  This is an
     exactly reproducible offset, not a proxy for rounding, so the driver is run a third time with the doubles and must give the same
     iteration counts and bad flags and stay within HALF of the comparison's tolerances (state 5e-7, chi2 0.5e-6 (1 + max |chi2|));
     the other half is left to rounding (observed 1e-12).  A case that fails either probe is given another seed.
  3. at least one hard_* case keeps >= 25 % of its edges active in pass 2 and runs >= 2 iterations there.
Build container only:  python tests/golden/make_ba_stereo_golden.py   (--search-hard FROM TO: list hard seeds that qualify)"""
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
import stereo_ba_synth  # noqa: E402

ORACLE = os.path.join(ROOT, "oracle")
OBJ = os.path.join(ORACLE, "_ref", "obj")
LIB = os.path.join(ORACLE, "_ref", "libba_stereo_ref.so")
SRC = os.path.join(HERE, "ba_stereo_ref.cpp")
GOLDEN = os.path.join(HERE, "ba_stereo_golden.npz")
OUTPUT_KEYS = ("poses", "points", "state", "chi2", "bad", "iters")
N_ITERS = 5
CHI2D, CHI3D = float(np.float32(5.99)), float(np.float32(7.815))


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
    L.ba_stereo_ref_optimize.restype = C.c_int
    L.ba_stereo_ref_optimize.argtypes = [C.c_int] * 3 + [C.c_void_p] * 10 + [C.c_int, C.c_double, C.c_int] + [C.c_void_p] * 11
    return L


def solve(L, pr, ur_shift=0.0, mono_limits_double=False):
    """The reference's outputs plus what the conditions look at (chi2_mid, z_mid, z_fin, zf_fin, active)."""
    P = oracle_lib.P
    K, Pn, E = pr["K"], pr["P"], pr["E"]
    o = dict(poses=np.zeros((K, 16), np.float32), points=np.zeros((Pn, 3), np.float32), chi2=np.zeros(E, np.float64), bad=np.zeros(E, np.uint8),
             iters=np.zeros(2, np.int32), state=np.zeros((K, 7), np.float64), chi2_mid=np.zeros(E, np.float64), z_mid=np.zeros(E, np.float64),
             z_fin=np.zeros(E, np.float64), zf_fin=np.zeros(E, np.float64), active=np.zeros(2, np.int32))
    rc = L.ba_stereo_ref_optimize(K, Pn, E, P(pr["poses"]), P(pr["fixed"]), P(pr["intr"]), P(pr["points"]), P(pr["obs_pt"]), P(pr["obs_kf"]),
                                  P(pr["obs_uv"]), P(pr["obs_w"]), P(pr["obs_depth"]), P(pr["frame_bl"]), N_ITERS, float(ur_shift), int(mono_limits_double), P(o["poses"]),
                                  P(o["points"]), P(o["chi2"]), P(o["bad"]), P(o["iters"]), P(o["state"]), P(o["chi2_mid"]), P(o["z_mid"]),
                                  P(o["z_fin"]), P(o["zf_fin"]), P(o["active"]))
    assert rc == 0
    return o


def input_digest(pr):
    return oracle_lib.digest(*[np.ascontiguousarray(pr[k]) for k in stereo_ba_synth.INPUT_KEYS])


def margins(L, pr, out):
    """(nearest relative distance of a chi2 to its limit, nearest |z| of a depth test to 0, state move under the 1e-9 px probe,
    probe keeps iterations and flags) — conditions 1 and 2."""
    st = pr["obs_depth"] > 0
    lim = np.where(st, CHI3D, CHI2D)
    chi = min(float((np.abs(out["chi2_mid"] - lim) / (1 + lim)).min()), float((np.abs(out["chi2"] - lim) / (1 + lim)).min()))
    zz = min(float(np.abs(out["z_mid"]).min()), float(np.abs(out["z_fin"][st]).min()) if st.any() else np.inf, float(np.abs(out["zf_fin"]).min()))
    pert = solve(L, pr, 1e-9)
    same = pert["iters"].tolist() == out["iters"].tolist() and bool((pert["bad"] == out["bad"]).all())
    return chi, zz, float(np.abs(pert["state"] - out["state"]).max()), same


def constants_probe(L, pr, out):
    """The driver with the product's monocular constants (doubles): (state move, chi2 move relative to 1 + max |chi2|, same iterations
    and flags) — the second half of condition 2."""
    alt = solve(L, pr, 0.0, True)
    same = alt["iters"].tolist() == out["iters"].tolist() and bool((alt["bad"] == out["bad"]).all())
    rel = float(np.abs(alt["chi2"] - out["chi2"]).max() / (1 + np.abs(out["chi2"]).max())) if pr["E"] else 0.0
    return float(np.abs(alt["state"] - out["state"]).max()), rel, same


def check_case(L, name, pr, out):
    chi, zz, move, same = margins(L, pr, out)
    print(f"{name}: K/P/E/stereo {pr['K']}/{pr['P']}/{pr['E']}/{int((pr['obs_depth'] > 0).sum())} iters {out['iters'].tolist()} bad {int(out['bad'].sum())} "
          f"active {out['active'].tolist()} | chi2-to-limit {chi:.2e} |z| {zz:.2e} probe move {move:.2e} same {same}")
    assert chi > 1e-6, f"{name}: condition 1 (an edge on its limit)"
    assert zz > 1e-9, f"{name}: condition 1 (a depth test on 0)"
    assert same and move < 1e-7, f"{name}: condition 2 (ill conditioned)"
    cmove, cchi, csame = constants_probe(L, pr, out)
    print(f"{name}: monocular constants as doubles: state move {cmove:.2e} chi2 move {cchi:.2e} (1 + max) same {csame}")
    assert csame and cmove < 5e-7 and cchi < 0.5e-6, f"{name}: condition 2 (the float / double monocular constants show)"


def hard_qualifies(out, E):
    return out["active"][1] >= 0.25 * E and out["iters"][1] >= 2


def generate():
    L = build_driver()
    save = {}
    hard_ok = False
    for name, kw in stereo_ba_synth.CASES.items():
        pr = stereo_ba_synth.stereo_ba_problem(**kw)
        out = solve(L, pr)
        check_case(L, name, pr, out)
        if name.startswith("hard_"):
            hard_ok = hard_ok or hard_qualifies(out, pr["E"])
        save[f"{name}_in_digest"] = input_digest(pr)
        for k in OUTPUT_KEYS:
            save[f"{name}_{k}"] = out[k]
    assert hard_ok, "condition 3: no hard_* case keeps >= 25 % of its edges in pass 2 for >= 2 iterations"
    return save


def search_hard(a, b):
    """Seeds whose problem shows what the hard cases are for (a pass that ends before its budget) and passes conditions 1-3."""
    L = build_driver()
    for seed in range(a, b):
        rng = np.random.default_rng(seed)
        kw = dict(K=int(rng.integers(5, 11)), P=int(rng.integers(60, 250)), seed=seed, **stereo_ba_synth.HARD)
        pr = stereo_ba_synth.stereo_ba_problem(**kw)
        out = solve(L, pr)
        early = out["iters"][0] < N_ITERS or out["iters"][1] < 2 * N_ITERS
        if not early or not hard_qualifies(out, pr["E"]):
            continue
        chi, zz, move, same = margins(L, pr, out)
        cmove, cchi, csame = constants_probe(L, pr, out)
        print(seed, kw["K"], kw["P"], pr["E"], out["iters"].tolist(), out["active"].tolist(), f"{chi:.1e} {zz:.1e} {move:.1e}", same, f"{cmove:.1e} {cchi:.1e}", csame,
              "OK" if chi > 1e-6 and zz > 1e-9 and same and move < 1e-7 and csame and cmove < 5e-7 and cchi < 0.5e-6 else "", flush=True)


if __name__ == "__main__":
    why = driver_available()
    assert why is None, why
    if len(sys.argv) > 1 and sys.argv[1] == "--search-hard":
        search_hard(int(sys.argv[2]), int(sys.argv[3]))
    else:
        np.savez_compressed(GOLDEN, **generate())
        print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
