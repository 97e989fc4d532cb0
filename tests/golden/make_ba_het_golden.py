"""Generates tests/golden/ba_het_golden.npz: bundle adjustment on windows of unequal cameras (tests/het_ba_synth.py) on the REAL
reference g2o, through the driver of tests/golden/make_ba_stereo_golden.py (ba_stereo_ref.cpp indexes intr[4 k] and frame_bl[k]).

Per case the fixture keeps a digest of the inputs and the reference's outputs; of the bench-size window (het_ba_synth.BENCH_CASE) only
the se3 state, the iteration counts and a SHA-256 of the flags.  Conditions 1 and 2 of make_ba_stereo_golden.py are asserted on every
case unchanged (check_case); a case that fails gets another seed.  On top of them:
  4. the fixture can see the faults it is for.  Every case is solved again as each of het_ba_synth.MUTANTS (row 0 of the intrinsics
     for all keyframes, fx and fy swapped, the first keyframe's baseline for all — cases with stereo edges —, the fixed flags moved
     to a prefix) and the se3 state must move by >= 1e-4, a hundred times the tolerance of the comparison.  A case below that gets a
     wider spread, not a lower bar.  The moves are printed (their minima per mutant: DESIGN.md §2).
Build container only:  python tests/golden/make_ba_het_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
import het_ba_synth  # noqa: E402
import make_ba_stereo_golden as S  # noqa: E402
import oracle_lib  # noqa: E402

GOLDEN = os.path.join(HERE, "ba_het_golden.npz")
MIN_MUTANT_MOVE = 1e-4

OUTPUT_KEYS = S.OUTPUT_KEYS
driver_available, input_digest = S.driver_available, S.input_digest


def mutant_moves(L, pr, out):
    """{mutant: (se3 state move, flags flipped)} with the real g2o — condition 4."""
    moves = {}
    for which in het_ba_synth.MUTANTS:
        if which == "bl0" and not (pr["obs_depth"] > 0).any():
            continue
        alt = S.solve(L, het_ba_synth.mutant(pr, which))
        moves[which] = (float(np.abs(alt["state"] - out["state"]).max()), int((alt["bad"] != out["bad"]).sum()))
    return moves


def check_mutants(L, name, pr, out):
    moves = mutant_moves(L, pr, out)
    print(f"{name}: mutants move the state by " + ", ".join(f"{k} {v[0]:.2e} ({v[1]} flags)" for k, v in moves.items()))
    for which, (move, _) in moves.items():
        assert move >= MIN_MUTANT_MOVE, f"{name}: condition 4 ({which} moves the state by {move:.2e} only)"
    return moves


def generate():
    L = S.build_driver()
    save, minima = {}, {}
    for name, kw in het_ba_synth.CASES.items():
        pr = het_ba_synth.het_ba_problem(**kw)
        out = S.solve(L, pr)
        S.check_case(L, name, pr, out)
        for which, (move, _) in check_mutants(L, name, pr, out).items():
            minima[which] = min(minima.get(which, np.inf), move)
        save[f"{name}_in_digest"] = input_digest(pr)
        for k in OUTPUT_KEYS:
            save[f"{name}_{k}"] = out[k]
    name, kw = het_ba_synth.BENCH_CASE
    pr = het_ba_synth.het_ba_problem(**kw)
    out = S.solve(L, pr)
    S.check_case(L, name, pr, out)
    for which, (move, _) in check_mutants(L, name, pr, out).items():
        minima[which] = min(minima.get(which, np.inf), move)
    save[f"{name}_in_digest"] = input_digest(pr)
    save[f"{name}_state"], save[f"{name}_iters"] = out["state"], out["iters"]
    save[f"{name}_bad_sha"], save[f"{name}_nbad"] = oracle_lib.digest(out["bad"]), np.int64(out["bad"].sum())
    print("condition 4, smallest state move per mutant: " + ", ".join(f"{k} {v:.2e}" for k, v in minima.items()))
    return save


if __name__ == "__main__":
    why = driver_available()
    assert why is None, why
    np.savez_compressed(GOLDEN, **generate())
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
