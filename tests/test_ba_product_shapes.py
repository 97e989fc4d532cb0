"""The persistent local BA's Schur product (schur_item_product, ba_persist.hpp) at the smallest windows on which its pipeline can go
wrong: a K-split with a tail behind its whole groups of four rows, a shorter last split, no tail at all, lanes without an item, partial
4 x 4 blocks, one landmark in the last workgroup, and the 16-lane instantiation with one and with three items per lane.
Every window is checked against the CPU oracle, against the launch chain (UH_BA_FORM=legacy) and against a second run of itself, with
the bars of test_ba.py."""
import numpy as np
import pytest

import oracle_lib
import synth

POSE_TOL = 1e-6   # test_ba.py

# (free keyframes, landmarks, persistent form): two fixed keyframes each.  plan_persist (ba.hip) gives, for Lw landmarks per workgroup,
# krows = 3 Lw rounded up to 16, nb4 = ceil(6 free / 4), nblk = nb4 (nb4 + 1) / 2 and the K-split count KS; kc = ceil(krows / KS).
CASES = [
    (8, 33, "persist8"),     # krows 32, 78 blocks, KS 3, kc 11: two groups + a tail of 3 rows, last split 10 rows; 5 workgroups, the last with one landmark
    (6, 33, "persist8"),     # the same splits on 45 blocks, n = 36
    (1, 33, "persist8"),     # 3 blocks, KS 4, kc 8: no tail, most lanes idle; n = 6 is not a multiple of 4
    (3, 130, "persist8"),    # n = 18: partial 4 x 4 blocks, 17 workgroups
    (1, 1300, "persist8"),   # krows 64, KS 6, kc 11, last split 9 rows
    (11, 33, "persist16"),   # 16 lanes per landmark, KS 1, kc 32
    (15, 33, "persist16"),   # 276 blocks x KS 2: three items per lane
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
def test_hip_ba_product_shapes(hip_ctx, oracle, monkeypatch, nfree, P, form):
    pr = synth.ba_problem(nfree + 2, P, 300 + 20 * nfree + P % 7, nfixed=2)
    ref = oracle_lib.ba_optimize(oracle, pr, 5)

    monkeypatch.delenv("UH_BA_FORM", raising=False)
    got, again, ran_as = _run(hip_ctx, pr)
    assert ran_as == form
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
