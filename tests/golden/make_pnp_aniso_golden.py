"""Generates tests/golden/pnp_aniso_golden.npz: pose-only PnP on an anisotropic camera whose principal point lies off the default
one (INTR below; every other PnP input of the suite has fx == fy == 718.856), on the REAL reference g2o.

  mono500 / mono1300 / mono3001     oracle/_ref/libg2o_ref.so, g2o_ref_pnp_solve (3001: beyond the solver's LDS-resident 3000 matches)
  mix500 / mix3001                  stereo / RGB-D matches, the driver of tests/golden/make_pnp_stereo_golden.py (pnp_stereo_ref.cpp)
The fixture keeps a digest of every case's inputs and the reference's outputs (pose, se3 state, bad flags, inliers, iterations).
Asserted per case: the same problem solved with fx and fy swapped moves the se3 state by >= 1e-4 (a hundred times the comparison's
tolerance), so a solver that swaps them cannot pass.  Build container only:  python tests/golden/make_pnp_aniso_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
import make_pnp_stereo_golden as S  # noqa: E402
import oracle_lib  # noqa: E402
import stereo_synth  # noqa: E402
import synth  # noqa: E402

GOLDEN = os.path.join(HERE, "pnp_aniso_golden.npz")
INTR = (655.1, 742.3, 633.7, 171.4)
MONO_CASES = {"mono500": dict(n=500, seed=41), "mono1300": dict(n=1300, seed=42), "mono3001": dict(n=3001, seed=43)}
STEREO_CASES = {"mix500": dict(n=500, seed=44), "mix3001": dict(n=3001, seed=45)}
OUTPUT_KEYS = S.OUTPUT_KEYS
MONO_INPUT_KEYS = ("pose", "intr", "p3d", "kp", "invsig", "weight")
MIN_SWAP_MOVE = 1e-4


def problem(name):
    if name in MONO_CASES:
        return synth.pnp_problem(intr=INTR, **MONO_CASES[name])
    return stereo_synth.stereo_pnp_problem(intr=INTR, **STEREO_CASES[name])


def swapped(pr):
    m = dict(pr)
    m["intr"] = np.ascontiguousarray(pr["intr"][[1, 0, 2, 3]])
    return m


def input_digest(name, pr):
    if name in MONO_CASES:
        return oracle_lib.digest(*[np.ascontiguousarray(pr[k], np.float32) for k in MONO_INPUT_KEYS])
    return S.input_digest(pr)


def driver_available():
    return S.driver_available() or (None if oracle_lib.load_ref("g2o") is not None else "oracle/_ref/libg2o_ref.so is not built (make -C oracle ref)")


def generate():
    g2o, L = oracle_lib.load_ref("g2o"), S.build_driver()

    def solve(name, pr):
        if name in MONO_CASES:
            out = oracle_lib.pnp_solve_ref(g2o, pr)
            out["ngood"] = np.int32(out["ngood"])
            return out
        return S.solve(L, pr)

    save = {}
    for name in list(MONO_CASES) + list(STEREO_CASES):
        pr = problem(name)
        out = solve(name, pr)
        move = float(np.abs(solve(name, swapped(pr))["state"] - out["state"]).max())
        print(f"{name}: n {pr['n']} ngood {int(out['ngood'])} iters {out['iters'].tolist()} | fx <-> fy moves the state by {move:.2e}")
        assert move >= MIN_SWAP_MOVE, (name, move)
        save[f"{name}_in_digest"] = input_digest(name, pr)
        for k in OUTPUT_KEYS:
            save[f"{name}_{k}"] = out[k]
    return save


if __name__ == "__main__":
    why = driver_available()
    assert why is None, why
    np.savez_compressed(GOLDEN, **generate())
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
