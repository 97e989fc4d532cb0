"""Generates tests/golden/posegraph_golden.npz: the loop-closure pose graph (graphoptsim3.cpp:74-168) on the REAL reference g2o.

The driver tests/golden/posegraph_ref.cpp is compiled against the g2o objects that `make -C oracle ref` leaves in oracle/_ref/obj/
(the reference tree's headers are needed as well) into oracle/_ref/libposegraph_ref.so, as C++17: its std::vectors and g2o's hold
fixed-size Eigen types, which a C++11 build with -mavx does not align.  Inputs: tests/posegraph_synth.py (CASES).

g2o differentiates the Sim3 edge numerically with a step of (double)1e-9f, so the reference's Jacobians carry rounding noise of about
2e-7 |t| and its own result is not reproducible below roughly 1e-5.  Every case is therefore solved at TWO steps, the reference's and
1e-4f, and for each the fixture keeps the outputs (poses, Sim3 state, iterations, Levenberg trials, lambda, chi2 before / after) and
how far the state and the chi2 move under the driver's eight jitter patterns (measurement translations times 1 +- 1e-12):
spread_state, spread_chi2.  The first linearisation (errors, both Jacobians, measurements) is kept for the 1e-4f step.

Admission, asserted on every case so that the GPU tests compare without an escape clause:
  1. at 1e-4f all eight jitters give the same iteration count and a state within SCREEN_TOL = 1e-8 of the unjittered one;
  2. at the reference's step they give the same iteration count and a state within REF_TOL = 1e-4;
  3. free-scale cases have at most 64 poses.
A case that fails is given another seed in posegraph_synth.CASES; at most one first-choice seed in three (posegraph_synth.FIRST_CHOICE)
may have been replaced — if more fail, the case design is wrong, not the seeds.
Build container only:  python tests/golden/make_posegraph_golden.py   (--check: regenerate and compare with the committed file;
--search NAME FROM TO: list the seeds of a case that qualify)"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, TESTS)
sys.path.insert(0, HERE)
import oracle_lib  # noqa: E402
import posegraph_synth  # noqa: E402
from make_ba_marker_golden import driver_available, reference_tree  # noqa: E402,F401

ORACLE = os.path.join(ROOT, "oracle")
OBJ = os.path.join(ORACLE, "_ref", "obj")
LIB = os.path.join(ORACLE, "_ref", "libposegraph_ref.so")
SRC = os.path.join(HERE, "posegraph_ref.cpp")
GOLDEN = os.path.join(HERE, "posegraph_golden.npz")
MAX_ITERS = 20
STEPS = {"d4": np.float32(1e-4), "ref": np.float32(0.0)}   # 0 = the driver leaves g2o's own _delta_der (1e-9f)
OUTPUT_KEYS = ("poses", "state", "iters", "trials", "info")
LIN_KEYS = ("lin_err", "lin_Ji", "lin_Jj", "meas")
JITTERS = range(1, 9)
SCREEN_TOL = 1e-8
REF_TOL = 1e-4
VP = C.c_void_p


class _In(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("n", "E", "idx_new", "idx_old", "fix_scale", "max_iters", "jitter")] + [("delta_der", C.c_float)] + \
               [(k, VP) for k in ("poses", "edge_i", "edge_j", "edge_w", "expected")]


_OUT_FIELDS = ("poses", "state", "iters", "trials", "info", "lin_err", "lin_Ji", "lin_Jj", "meas", "seconds")


class _Out(C.Structure):
    _fields_ = [(k, VP) for k in _OUT_FIELDS]


def build_driver():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < os.path.getmtime(SRC):
        ref = reference_tree()
        g2o = os.path.join(ref, "3rdparty", "g2o")
        objs = sorted(os.path.join(OBJ, f) for f in os.listdir(OBJ) if f.endswith(".o"))
        cmd = ["g++", "-std=c++17", "-O3", "-mavx", "-msse3", "-mpopcnt", "-fPIC", "-w", "-DNDEBUG", f"-I{g2o}",
               f"-I{os.path.join(ref, '3rdparty', 'eigen3', 'eigen3')}", f"-I{os.path.join(g2o, 'g2o', 'stuff')}", "-shared", "-o", LIB, SRC,
               *objs, "-lpthread"]
        subprocess.check_call(cmd)
    L = C.CDLL(LIB)
    L.posegraph_ref_optimize.restype = C.c_int
    L.posegraph_ref_optimize.argtypes = [C.POINTER(_In), C.POINTER(_Out)]
    return L


def solve(L, pr, delta_der=0.0, jitter=0, max_iters=MAX_ITERS):
    P = oracle_lib.P
    n, E = pr["n"], pr["E"]
    o = dict(poses=np.zeros((n, 16), np.float32), state=np.zeros((n, 8), np.float64), iters=np.zeros(1, np.int32), trials=np.zeros(max_iters, np.int32),
             info=np.zeros(3, np.float64), lin_err=np.zeros((E, 7), np.float64), lin_Ji=np.zeros((E, 7, 7), np.float64),
             lin_Jj=np.zeros((E, 7, 7), np.float64), meas=np.zeros((E, 8), np.float64), seconds=np.zeros(1, np.float64))
    a = {k: np.ascontiguousarray(pr[k]) for k in INPUT_ARRAYS}
    i = _In(n, E, pr["idx_new"], pr["idx_old"], pr["fix_scale"], max_iters, int(jitter), float(delta_der), P(a["poses"]), P(a["edge_i"]), P(a["edge_j"]),
            P(a["edge_w"]) if len(a["edge_w"]) else None, P(a["expected"]))
    oo = _Out(*[P(o[k]) for k in _OUT_FIELDS])
    assert L.posegraph_ref_optimize(C.byref(i), C.byref(oo)) == 0
    return o


INPUT_ARRAYS = ("poses", "edge_i", "edge_j", "edge_w", "expected")


def input_digest(pr):
    return oracle_lib.digest(*[np.ascontiguousarray(pr[k]) for k in posegraph_synth.INPUT_KEYS], np.array([pr["fix_scale"]], np.int32))


def rel_chi2(a, b):
    return float(np.abs(a["info"][1:] - b["info"][1:]).max() / (1 + np.abs(b["info"][1:]).max()))


def spreads(L, pr, out, delta_der):
    """(why not admitted or None, state spread, chi2 spread) of one step over the eight jitters."""
    ss, sc = 0.0, 0.0
    for j in JITTERS:
        jo = solve(L, pr, delta_der, j)
        if int(jo["iters"][0]) != int(out["iters"][0]):
            return f"jitter {j}: iterations {int(jo['iters'][0])} != {int(out['iters'][0])}", ss, sc
        ss = max(ss, float(np.abs(jo["state"] - out["state"]).max()))
        sc = max(sc, rel_chi2(jo, out))
    return None, ss, sc


def case_outputs(L, pr):
    """{key: array} of one case at both steps, and why it is not admitted (or None)."""
    if not pr["fix_scale"] and pr["n"] > 64:
        return {}, "a free-scale case with more than 64 poses"
    save, why = {}, None
    for tag, dd in STEPS.items():
        out = solve(L, pr, dd)
        if not (np.isfinite(out["state"]).all() and np.isfinite(out["info"]).all()):
            return save, f"{tag}: non-finite outputs"
        w, ss, sc = spreads(L, pr, out, dd)
        if w:
            return save, f"{tag}: {w}"
        tol = SCREEN_TOL if tag == "d4" else REF_TOL
        if not ss <= tol:
            return save, f"{tag}: the state moves by {ss:.3g} > {tol:g} under the jitters"
        for k in OUTPUT_KEYS:
            save[f"{tag}_{k}"] = out[k]
        if tag == "d4":
            for k in LIN_KEYS:
                save[f"{tag}_{k}"] = out[k]
        save[f"{tag}_spread_state"] = np.float64(ss)
        save[f"{tag}_spread_chi2"] = np.float64(sc)
    return save, why


def generate(verbose=True):
    L = build_driver()
    save = {}
    cases = posegraph_synth.CASES
    replaced = [n for n, kw in cases.items() if kw["seed"] != posegraph_synth.FIRST_CHOICE[n]]
    if verbose:
        print(f"{len(replaced)} of {len(cases)} first-choice seeds replaced by the screen: {replaced}")
    assert 3 * len(replaced) <= len(cases), "more than one first-choice seed in three replaced: the case design is wrong, not the seeds"
    for name, kw in cases.items():
        pr = posegraph_synth.posegraph_problem(**kw)
        out, why = case_outputs(L, pr)
        assert why is None, f"case {name} (seed {kw['seed']}): {why} — replace its seed in posegraph_synth.CASES"
        if verbose:
            print(f"{name}: n/E {pr['n']}/{pr['E']} fix_scale {pr['fix_scale']} | 1e-4f: iters {int(out['d4_iters'][0])} trials {out['d4_trials'][:int(out['d4_iters'][0])].tolist()} "
                  f"chi2 {out['d4_info'][1]:.4g} -> {out['d4_info'][2]:.4g} spread {float(out['d4_spread_state']):.2e} / {float(out['d4_spread_chi2']):.2e} | "
                  f"reference step: iters {int(out['ref_iters'][0])} spread {float(out['ref_spread_state']):.2e} / {float(out['ref_spread_chi2']):.2e}")
        save[f"{name}_in_digest"] = input_digest(pr)
        for k, v in out.items():
            save[f"{name}_{k}"] = v
    return save


def check():
    """Regenerate and compare with the committed file: digests and integers exactly, floating-point outputs to 1e-12 (1 + |v|) at the
    1e-4f step (the same binary on another CPU may contract or vectorise differently) and to the case's own spread at the reference's."""
    old = np.load(GOLDEN)
    new = generate(verbose=False)
    assert sorted(old.files) == sorted(new), "the fixture's keys differ"
    for k in old.files:
        a, b = old[k], np.asarray(new[k])
        if a.dtype.kind in "iu":
            assert np.array_equal(a, b), k
        elif "spread" in k:
            continue
        else:
            name = next(n for n in posegraph_synth.CASES if k.startswith(n + "_"))
            tol = 1e-12 if f"{name}_d4_" in k else 10 * float(old[f"{name}_ref_spread_state"]) + 1e-12
            if k.endswith("_info"):   # lambda (tiny) and the chi2 pair: relative
                assert np.allclose(a, b, rtol=1e-6 if "_ref_" in k else 1e-9, atol=1e-30), (k, a, b)
            else:
                assert (np.abs(a.astype(np.float64) - b.astype(np.float64)) <= tol * (1 + np.abs(a.astype(np.float64))) + (1.2e-7 * np.abs(a) if a.dtype == np.float32 else 0)).all(), k
    print("posegraph_golden.npz reproduced")


def search(name, a, b):
    L = build_driver()
    for seed in range(a, b):
        kw = dict(posegraph_synth.CASES[name], seed=seed)
        _, why = case_outputs(L, posegraph_synth.posegraph_problem(**kw))
        print(seed, why or "OK", flush=True)


if __name__ == "__main__":
    why = driver_available()
    assert why is None, why
    if len(sys.argv) > 1 and sys.argv[1] == "--search":
        search(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    elif len(sys.argv) > 1 and sys.argv[1] == "--check":
        check()
    else:
        np.savez_compressed(GOLDEN, **generate())
        print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
