"""Generates tests/golden/ba_marker_golden.npz: bundle adjustment with keypoint observations and free marker poses on the REAL reference g2o.

The driver tests/golden/ba_marker_ref.cpp is compiled against the g2o objects that `make -C oracle ref` leaves in oracle/_ref/obj/
(the reference tree's headers are needed as well) into oracle/_ref/libba_marker_ref.so.  Inputs: tests/ba_marker_synth.py (CASES);
the fixture keeps a digest of every case's inputs, the reference's outputs (poses, marker poses, points, the se3 state of frames and
markers, chi2 of keypoint and marker edges, bad flags, iterations) and, for the first linearisation only, every marker edge's error
and both Jacobians as g2o's own numeric linearizeOplus leaves them.

Conditions asserted on every case, so that the GPU tests compare without an escape clause (margins are printed):
  1. make_ba_stereo_golden.py's: no keypoint edge's between-pass or final chi2 within 1e-6 (1 + limit) of its limit, no depth test
     within 1e-9 of 0; the kp_ur probe (+-1e-9 px) and the monocular-constants probe (the limits as doubles) keep iterations and flags,
     the former with the state within 1e-7, the latter within HALF of the comparison's tolerances (state 5e-7, chi2 0.5e-6 (1 + max)).
  2. make_pnp_marker_golden.py's jitter screen, because the marker edge rounds its projections to float and is differentiated
     numerically, so the reference itself is discontinuous: the driver's eight jitter patterns (camera-frame corner coordinates times
     1 +- 1e-11, 1 +- 0.7e-11 for z) all give the same iterations, the same bad flags and a state (frames and markers) within
     SCREEN_TOL of the unjittered one.
A case that fails is given another seed in ba_marker_synth.CASES; at most one first-choice seed in three (ba_marker_synth.FIRST_CHOICE)
may have been replaced — if more fail, the case design is wrong, not the seeds.  generate() prints how many were.
Build container only:  python tests/golden/make_ba_marker_golden.py   (--search NAME FROM TO: list the seeds of a case that qualify)"""
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
import ba_marker_synth  # noqa: E402
import oracle_lib  # noqa: E402

ORACLE = os.path.join(ROOT, "oracle")
OBJ = os.path.join(ORACLE, "_ref", "obj")
LIB = os.path.join(ORACLE, "_ref", "libba_marker_ref.so")
SRC = os.path.join(HERE, "ba_marker_ref.cpp")
GOLDEN = os.path.join(HERE, "ba_marker_golden.npz")
OUTPUT_KEYS = ("state", "marker_state", "poses", "marker_poses", "points", "chi2", "marker_chi2", "bad", "iters", "trials", "lin_err", "lin_Ji", "lin_Jj")
N_ITERS = 5
CHI2D, CHI3D = float(np.float32(5.99)), float(np.float32(7.815))
JITTERS = range(1, 9)
SCREEN_TOL = 1e-9
VP = C.c_void_p


class _In(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("K", "P", "E", "M", "EM", "nIters")] + \
               [(k, VP) for k in ("poses_f2g", "fixed", "intr", "points", "obs_pt", "obs_kf", "obs_uv", "obs_invsigma", "obs_depth", "frame_bl",
                                  "mk_pose", "mk_size", "me_marker", "me_frame", "me_corners", "me_weight")] + \
               [("ur_shift", C.c_double), ("mono_limits_double", C.c_int32), ("jitter", C.c_int32)]


_OUT_FIELDS = ("poses", "points", "chi2", "bad", "iters", "state", "marker_poses", "marker_state", "marker_chi2", "lin_err", "lin_Ji", "lin_Jj",
               "chi2_mid", "z_mid", "z_fin", "zf_fin", "active", "trials")


class _Out(C.Structure):
    _fields_ = [(k, VP) for k in _OUT_FIELDS]


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
    L.ba_marker_ref_optimize.restype = C.c_int
    L.ba_marker_ref_optimize.argtypes = [C.POINTER(_In), C.POINTER(_Out)]
    return L


def solve(L, pr, ur_shift=0.0, mono_limits_double=False, jitter=0):
    """The reference's outputs plus what the conditions look at (chi2_mid, z_mid, z_fin, zf_fin, active)."""
    P = oracle_lib.P
    K, Pn, E, M, EM = pr["K"], pr["P"], pr["E"], pr["M"], pr["EM"]
    o = dict(poses=np.zeros((K, 16), np.float32), points=np.zeros((Pn, 3), np.float32), chi2=np.zeros(E, np.float64), bad=np.zeros(E, np.uint8),
             iters=np.zeros(2, np.int32), state=np.zeros((K, 7), np.float64), marker_poses=np.zeros((M, 16), np.float32),
             marker_state=np.zeros((M, 7), np.float64), marker_chi2=np.zeros(EM, np.float64), lin_err=np.zeros((EM, 8), np.float64),
             lin_Ji=np.zeros((EM, 8, 6), np.float64), lin_Jj=np.zeros((EM, 8, 6), np.float64), chi2_mid=np.zeros(E, np.float64),
             z_mid=np.zeros(E, np.float64), z_fin=np.zeros(E, np.float64), zf_fin=np.zeros(E, np.float64), active=np.zeros(2, np.int32), trials=np.zeros(2, np.int32))
    a = {k: np.ascontiguousarray(pr[k]) for k in ba_marker_synth.INPUT_KEYS + ba_marker_synth.MARKER_KEYS}
    i = _In(K, Pn, E, M, EM, N_ITERS, P(a["poses"]), P(a["fixed"]), P(a["intr"]), P(a["points"]), P(a["obs_pt"]), P(a["obs_kf"]), P(a["obs_uv"]),
            P(a["obs_w"]), P(a["obs_depth"]), P(a["frame_bl"]), P(a["mk_pose"]), P(a["mk_size"]), P(a["me_marker"]), P(a["me_frame"]),
            P(a["me_corners"]), P(a["me_weight"]), float(ur_shift), int(mono_limits_double), int(jitter))
    oo = _Out(*[P(o[k]) for k in _OUT_FIELDS])
    assert L.ba_marker_ref_optimize(C.byref(i), C.byref(oo)) == 0
    return o


def input_digest(pr):
    return oracle_lib.digest(*[np.ascontiguousarray(pr[k]) for k in ba_marker_synth.INPUT_KEYS + ba_marker_synth.MARKER_KEYS])


def _full_state(o):
    return np.concatenate([o["state"].ravel(), o["marker_state"].ravel()])


def _same(a, b):
    return a["iters"].tolist() == b["iters"].tolist() and bool((a["bad"] == b["bad"]).all())


def _rel_chi2(a, b):
    ca, cb = np.concatenate([a["chi2"], a["marker_chi2"]]), np.concatenate([b["chi2"], b["marker_chi2"]])
    return float(np.abs(ca - cb).max() / (1 + np.abs(cb).max()))


def why_not(L, pr, out, say=None):
    """None when the case passes every condition, else the first one it fails."""
    if not (np.isfinite(_full_state(out)).all() and np.isfinite(out["chi2"]).all() and np.isfinite(out["marker_chi2"]).all()):
        return "non-finite outputs"
    if pr["E"]:
        st = pr["obs_depth"] > 0
        lim = np.where(st, CHI3D, CHI2D)
        chi = min(float((np.abs(out["chi2_mid"] - lim) / (1 + lim)).min()), float((np.abs(out["chi2"] - lim) / (1 + lim)).min()))
        zz = min(float(np.abs(out["z_mid"]).min()), float(np.abs(out["z_fin"][st]).min()) if st.any() else np.inf, float(np.abs(out["zf_fin"]).min()))
        if not chi > 1e-6:
            return f"condition 1 (an edge on its limit: {chi:.2e})"
        if not zz > 1e-9:
            return f"condition 1 (a depth test on 0: {zz:.2e})"
        pert = solve(L, pr, 1e-9)
        move = float(np.abs(_full_state(pert) - _full_state(out)).max())
        if not (_same(pert, out) and move < 1e-7):
            return f"condition 1 (ill conditioned: kp_ur probe moves the state by {move:.2e}, same {_same(pert, out)})"
        alt = solve(L, pr, 0.0, True)
        cmove, cchi = float(np.abs(_full_state(alt) - _full_state(out)).max()), _rel_chi2(alt, out)
        if not (_same(alt, out) and cmove < 5e-7 and cchi < 0.5e-6):
            return f"condition 1 (the float / double monocular constants show: state {cmove:.2e} chi2 {cchi:.2e} same {_same(alt, out)})"
        if say is not None:
            say(f"chi2-to-limit {chi:.2e} |z| {zz:.2e} kp_ur probe {move:.2e} constants probe {cmove:.2e} / {cchi:.2e}")
    worst = 0.0
    for j in JITTERS:
        jo = solve(L, pr, jitter=j)
        if jo["iters"].tolist() != out["iters"].tolist():
            return f"condition 2 (jitter {j}: iterations {jo['iters'].tolist()} != {out['iters'].tolist()})"
        if not np.array_equal(jo["bad"], out["bad"]):
            return f"condition 2 (jitter {j}: {int((jo['bad'] != out['bad']).sum())} bad flags differ)"
        d = float(np.abs(_full_state(jo) - _full_state(out)).max())
        worst = max(worst, d)
        if not d <= SCREEN_TOL:
            return f"condition 2 (jitter {j}: state moves by {d:.3g} > {SCREEN_TOL:g})"
    if say is not None:
        say(f"jitter screen: state moves by at most {worst:.2e}")
    return None


def generate():
    L = build_driver()
    save = {}
    replaced = [n for n, kw in ba_marker_synth.CASES.items() if kw["seed"] != ba_marker_synth.FIRST_CHOICE[n]]
    print(f"{len(replaced)} of {len(ba_marker_synth.CASES)} first-choice seeds replaced by the screen: {replaced}")
    assert 3 * len(replaced) <= len(ba_marker_synth.CASES), "more than one first-choice seed in three replaced: the case design is wrong, not the seeds"
    for name, kw in ba_marker_synth.CASES.items():
        pr = ba_marker_synth.marker_ba_problem(**kw)
        out = solve(L, pr)
        print(f"{name}: K/P/E {pr['K']}/{pr['P']}/{pr['E']} stereo {int((pr['obs_depth'] > 0).sum())} markers {pr['M']} marker edges {pr['EM']} "
              f"iters {out['iters'].tolist()} trials {out['trials'].tolist()} bad {int(out['bad'].sum())} active {out['active'].tolist()} weights {np.unique(pr['me_weight']).round(4).tolist()}")
        why = why_not(L, pr, out, say=lambda s: print(f"{name}: {s}"))
        assert why is None, f"case {name} (seed {kw['seed']}): {why} — replace its seed in ba_marker_synth.CASES"
        if name == "mk_hard":
            assert (out["trials"] > out["iters"]).any(), "mk_hard: no Levenberg trial was rejected"
        save[f"{name}_in_digest"] = input_digest(pr)
        for k in OUTPUT_KEYS:
            save[f"{name}_{k}"] = out[k]
    assert any(save[f"{n}_iters"].tolist() != [N_ITERS, 2 * N_ITERS] for n in ba_marker_synth.CASES), "no case ends a pass before its budget"
    return save


def search(name, a, b):
    """Seeds with which case `name` passes every condition."""
    L = build_driver()
    for seed in range(a, b):
        kw = dict(ba_marker_synth.CASES[name], seed=seed)
        pr = ba_marker_synth.marker_ba_problem(**kw)
        out = solve(L, pr)
        print(seed, out["iters"].tolist(), out["trials"].tolist(), int(out["bad"].sum()), why_not(L, pr, out) or "OK", flush=True)


if __name__ == "__main__":
    why = driver_available()
    assert why is None, why
    if len(sys.argv) > 1 and sys.argv[1] == "--search":
        search(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    else:
        np.savez_compressed(GOLDEN, **generate())
        print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
