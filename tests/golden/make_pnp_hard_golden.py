"""Generates tests/golden/pnp_hard_golden.npz: pose-only PnP driven through the solver's rarely taken branches, on the REAL reference g2o.

The driver is the second entry point of tests/golden/pnp_stereo_ref.cpp (pnp_hard_ref_solve, built by make_pnp_stereo_golden.py's recipe
into oracle/_ref/libpnp_stereo_ref.so): the same graph and loop, plus the Levenberg trials of every iteration as g2o counts them and an
optional jitter of the map points.  Inputs: tests/pnp_hard_synth.py (CASES); the fixture keeps a digest of every case's inputs and the
reference's outputs (pose, se3 state, bad flags, inliers, iterations per round, trials per round and iteration).

The screen (asserted for every case): a case whose reference outcome hangs on rounding noise cannot pin a solver, so the driver is run
again with each of 8 seeded relative 1e-12 perturbations of the map points (in its doubles); iterations, trials, bad flags and the inlier
count must not change and the state must stay within SCREEN_TOL (non-finite entries in the same places).  pnp_hard_synth.CASES lists,
per case, every seed that reached the case's state and was put to this screen (`tried`); the screen may reject at most half of them —
if it rejects more, the case design is wrong, not the seeds.  generate() screens them all again, asserts both and prints the counts.
Build container only:  python tests/golden/make_pnp_hard_golden.py   (--search NAME FROM TO: the seeds of a case and what the screen says)"""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
import oracle_lib  # noqa: E402
import pnp_hard_synth  # noqa: E402

GOLDEN = os.path.join(HERE, "pnp_hard_golden.npz")
OUTPUT_KEYS = ("pose", "state", "bad", "ngood", "iters", "trials")
JITTERS = range(1, 9)
SCREEN_TOL = 1e-9


def _stereo_gen():
    spec = importlib.util.spec_from_file_location("make_pnp_stereo_golden", os.path.join(HERE, "make_pnp_stereo_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def driver_available():
    """Why the driver cannot be built here, or None when it can."""
    return _stereo_gen().driver_available()


def build_driver():
    L = _stereo_gen().build_driver()
    L.pnp_hard_ref_solve.restype = C.c_int
    L.pnp_hard_ref_solve.argtypes = [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 5 + [C.c_float, C.c_int] + [C.c_void_p] * 5
    return L


def solve(L, pr, jitter=0):
    P = oracle_lib.P
    a = {k: np.ascontiguousarray(pr[k], np.float32) for k in pnp_hard_synth.INPUT_KEYS}
    n = len(a["invsig"])
    pose = np.zeros(16, np.float32)
    bad = np.zeros(max(n, 1), np.uint8)
    iters = np.zeros(4, np.int32)
    trials = np.zeros((4, 10), np.int32)
    state = np.zeros(7, np.float64)
    ngood = L.pnp_hard_ref_solve(P(a["pose"]), P(a["intr"]), n, P(a["p3d"]), P(a["kp"]), P(a["invsig"]), P(a["weight"]), P(a["depth"]),
                                 float(pr["bl"]), int(jitter), P(pose), P(bad), P(iters), P(state), P(trials))
    return dict(pose=pose, state=state, bad=bad[:n], ngood=np.int32(ngood), iters=iters, trials=trials)


def input_digest(pr):
    return oracle_lib.digest(*[np.ascontiguousarray(pr[k], np.float32) for k in pnp_hard_synth.INPUT_KEYS], np.float32(pr["bl"]))


def state_distance(a, b):
    """max |a - b| over the finite entries; inf when the non-finite entries are not the same ones in the same places."""
    fa, fb = np.isfinite(a), np.isfinite(b)
    if not np.array_equal(fa, fb) or not np.array_equal(a[~fa], b[~fb], equal_nan=True):
        return np.inf
    return float(np.abs(a[fa] - b[fb]).max()) if fa.any() else 0.0


def why_not(L, pr, out, say=None):
    """None when the case passes the screen, else the first jitter it fails at."""
    worst = 0.0
    for j in JITTERS:
        jo = solve(L, pr, jitter=j)
        for k in ("iters", "trials", "bad"):
            if not np.array_equal(jo[k], out[k]):
                return f"jitter {j}: {k} differ"
        if int(jo["ngood"]) != int(out["ngood"]):
            return f"jitter {j}: {int(jo['ngood'])} inliers != {int(out['ngood'])}"
        d = state_distance(jo["state"], out["state"])
        worst = max(worst, d)
        if not d <= SCREEN_TOL:
            return f"jitter {j}: state moves by {d:.3g} > {SCREEN_TOL:g}"
    if say is not None:
        say(f"jitter screen: state moves by at most {worst:.2e}")
    return None


def generate(screen_all_tried=False):
    """The fixture's entries; every case's own seed is screened.  screen_all_tried: every seed of `tried` is, and the rejections are counted."""
    L = build_driver()
    save = {}
    tried, rejected = {}, {}
    for name, case in pnp_hard_synth.CASES.items():
        assert case["seed"] in case["tried"], name
        for seed in (case["tried"] if screen_all_tried else [case["seed"]]):
            pr = pnp_hard_synth.case_problem(name, seed)
            out = solve(L, pr)
            why = why_not(L, pr, out, say=(lambda s: print(f"{name}: {s}")) if seed == case["seed"] else None)
            tried.setdefault(case["state"], []).append((name, seed))
            if why is not None:
                rejected.setdefault(case["state"], []).append((name, seed))
                print(f"{name}: seed {seed} rejected by the screen ({why})")
            if seed != case["seed"]:
                continue
            assert why is None, f"case {name} (seed {seed}): {why} — choose another of its seeds in pnp_hard_synth.CASES"
            print(f"{name}: n {len(pr['invsig'])} stereo {int((pr['depth'] > 0).sum())} ngood {int(out['ngood'])} iters {out['iters'].tolist()} "
                  f"trials {[t[:i].tolist() for t, i in zip(out['trials'], out['iters'])]} finite {bool(np.isfinite(out['state']).all())}")
            save[f"{name}_in_digest"] = input_digest(pr)
            for k in OUTPUT_KEYS:
                save[f"{name}_{k}"] = out[k]
    for state, t in tried.items() if screen_all_tried else ():
        r = rejected.get(state, [])
        print(f"state '{state}': {len(t)} seeds tried, {len(r)} rejected by the screen {[f'{n}:{s}' for n, s in r]}")
        assert 2 * len(r) <= len(t), f"state '{state}': the screen rejects more than half of the seeds tried: the case design is wrong, not the seeds"
    return save


def search(name, a, b):
    """Seeds a..b-1 of case `name`: the reference's outcome and what the screen says."""
    L = build_driver()
    for seed in range(a, b):
        pr = pnp_hard_synth.case_problem(name, seed)
        out = solve(L, pr)
        print(seed, int(out["ngood"]), out["iters"].tolist(), [t[:i].tolist() for t, i in zip(out["trials"], out["iters"])], why_not(L, pr, out) or "OK", flush=True)


if __name__ == "__main__":
    why = driver_available()
    assert why is None, why
    if len(sys.argv) > 1 and sys.argv[1] == "--search":
        search(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    else:
        np.savez_compressed(GOLDEN, **generate(screen_all_tried=True))
        print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
