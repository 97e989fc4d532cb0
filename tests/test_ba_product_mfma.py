"""The persistent local BA's Schur product on the f64 matrix pipe (schur_product_mfma, ba_persist.hpp) at the windows that are specific
to 16 x 16 tiles: one tile partly used, a second or third tile row that is nearly empty or partly used, two / three / six k-steps per
wave, and the 16-lane instantiation's three tile lists (four, five and six tile rows dealt to the waves), the last with a partial
last workgroup.  test_ba_product_shapes.py runs the same code at its seven windows; this file adds what depends on tiles.
Every window is checked against the CPU oracle, against the launch chain (UH_BA_FORM=legacy) and against a second run of itself, with
the bars of test_ba_product_shapes.py.  The seeds are a formula of the window, fixed before the first run; the commit before the
MFMA product passes every window with them."""
import numpy as np
import pytest

import oracle_lib
import synth

POSE_TOL = 1e-6   # test_ba.py

# (free keyframes, landmarks, persistent form): two fixed keyframes each.  n = 6 free columns, NTT = ceil(n / 16) tile rows; plan_persist
# (ba.hip) gives Lw landmarks per workgroup and krows = 3 Lw rounded up to 16; up to three tile rows every wave takes krows / 16 k-steps.
CASES = [
    (2, 40, "persist8"),      # n = 12: one tile, partly used
    (3, 40, "persist8"),      # n = 18: two tile rows, the second nearly empty
    (5, 200, "persist8"),     # n = 30
    (6, 40, "persist8"),      # n = 36: three tile rows, the last partly used
    (8, 700, "persist8"),     # krows 48: three k-steps per wave
    (8, 2048, "persist8"),    # krows 96: the workload's split, 64 workgroups, six k-steps per wave
    (9, 33, "persist16"),     # four tile rows: ten tiles dealt 3 3 2 2
    (13, 33, "persist16"),    # five tile rows: fifteen tiles
    (16, 130, "persist16"),   # six tile rows: 21 tiles dealt 6 5 5 5; the last workgroup is partial
]


def _run(ctx, pr):
    from ucoslam_cv3_amd.ba import GlobalOptimizer, ParamSet

    opt = GlobalOptimizer.create(ctx)
    opt.setParams(pr, ParamSet(nIters=5))
    opt.optimize()
    first = opt.getResults()
    form = opt.form()
    opt.optimize()
    return first, opt.getResults(), form


@pytest.mark.gpu
@pytest.mark.parametrize("nfree,P,form", CASES, ids=lambda v: str(v))
def test_hip_ba_product_mfma(hip_ctx, oracle, monkeypatch, nfree, P, form):
    pr = synth.ba_problem(nfree + 2, P, 700 + 20 * nfree + P % 7, nfixed=2)
    ref = oracle_lib.ba_optimize(oracle, pr, 5)

    monkeypatch.delenv("UH_BA_FORM", raising=False)
    got, again, ran_as = _run(hip_ctx, pr)
    assert ran_as == form
    assert ran_as in ("persist8", "persist16")
    monkeypatch.setenv("UH_BA_FORM", "legacy")
    chain, _, chain_as = _run(hip_ctx, pr)
    assert chain_as == "chain"

    err = {k: float(np.abs(got[k] - ref[k]).max()) for k in ("state", "poses", "points")}
    vs_chain = float(np.abs(got["state"] - chain["state"]).max())
    print(f"free {nfree} P {P} {ran_as}: iters {got['iters'].tolist()} | against the oracle {err} | against the launch chain {vs_chain:.3g}")
    # the CPU oracle
    assert got["iters"].tolist() == ref["iters"].tolist()
    assert err["state"] < POSE_TOL
    assert err["poses"] < 1e-5 and err["points"] < 1e-4   # float32 outputs
    np.testing.assert_array_equal(got["bad"], ref["bad"])
    # the launch chain
    assert chain["iters"].tolist() == got["iters"].tolist()
    assert vs_chain < 1e-9
    np.testing.assert_array_equal(chain["bad"], got["bad"])
    # a second run from the same snapshot: bit-identical
    for k in ("state", "poses", "points", "bad", "iters"):
        np.testing.assert_array_equal(again[k], got[k])
