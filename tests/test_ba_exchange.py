"""The persistent local BA's exchange fetch (tld_raw / tload8, ba_persist.hpp: one 16-byte L2-bypassing load per tagged element, a failed
poll re-issues only what has not matched) at the smallest windows on which it can go wrong: a lone workgroup that reduces its own
partial, a second workgroup with one live landmark, a last source batch of fewer than eight, the maximal fan-in with the shortest slices,
the bench's window, the 16-lane instantiation (the reduced vector in more than one batch of eight), and hand-off C (the decision's poll of
chi2 / scale pairs) in a pass's last trial and in every trial.
Every window is checked against the launch chain (UH_BA_FORM=legacy) with the bars test_ba.py sets between forms, and against a second
run of itself, bit for bit; the form that ran is asserted, so a fallback to the launch chain cannot pass."""
import numpy as np
import pytest

import synth

SEED = 700   # with this seed every requested landmark keeps >= 2 observations at each size below (asserted): P is exactly what the row says

# (free keyframes, landmarks, UH_BA_LW, nIters, UH_BA_SPEC, form, workgroups): two fixed keyframes each.  plan_persist (ba.hip): G =
# ceil(P / Lw) workgroups, nelem exchanged elements, slices of SL = ceil(nelem / G) rounded up to even, HG = min(G, 256 / SL) source groups.
CASES = [
    (1, 1, None, 5, None, "persist8", 1),        # G = 1: a reducer whose only source is itself, HG = 1
    (3, 9, 8, 5, None, "persist8", 2),           # second workgroup with one live landmark; product entries beyond n are never sent (need bits clear)
    (8, 257, 8, 5, None, "persist8", 33),        # cnt < 8 in the last source batch, padded last slice
    (8, 2048, 8, 5, None, "persist8", 256),      # maximal fan-in, smallest SL
    (8, 3000, None, 5, None, "persist8", 94),    # the bench's window
    (9, 300, None, 5, None, "persist16", None),  # ba_persist_kernel<16>: the reduced vector arrives in more than one batch of eight
    (16, 500, None, 5, None, "persist16", None), # the same at the widest system
    (8, 300, None, 1, None, "persist8", None),   # nIters = 1: the trial that is its pass's last, hand-off C
    (8, 300, None, 5, "0", "persist8", None),    # UH_BA_SPEC=0: hand-off C in every trial
]


def _bad_flags_equal_up_to_the_boundary(got, ref, chi2_th=5.99):
    """test_ba.py's rule between two implementations: identical flags, except where chi2 lies within 1e-6 (relative) of the threshold."""
    diff = np.nonzero(got["bad"] != ref["bad"])[0]
    on_boundary = np.abs(ref["chi2"][diff] - chi2_th) <= 1e-6 * (1 + chi2_th)
    assert on_boundary.all(), f"{(~on_boundary).sum()} bad-association flags differ away from the chi2 = {chi2_th} boundary"


def _run(ctx, pr, n_iters):
    from ucoslam_cv3_amd.ba import GlobalOptimizer, ParamSet

    opt = GlobalOptimizer.create(ctx)
    opt.setParams(pr, ParamSet(nIters=n_iters))
    opt.optimize()
    first = opt.getResults()
    form = opt.form()
    opt.optimize()
    again = opt.getResults()
    opt.close()
    return first, again, form


@pytest.mark.gpu
@pytest.mark.parametrize("nfree,P,lw,n_iters,spec,form,G", CASES, ids=lambda v: str(v))
def test_hip_ba_exchange_fetch(hip_ctx, monkeypatch, nfree, P, lw, n_iters, spec, form, G):
    pr = synth.ba_problem(nfree + 2, P, SEED, nfixed=2)
    assert pr["P"] == P
    lw_eff = lw if lw is not None else max(8, min(256 // (8 if nfree <= 8 else 16), -(-P // 64)))
    if G is not None:
        assert -(-P // lw_eff) == G   # the row reaches the workgroup count it names

    for k in ("UH_BA_FORM", "UH_BA_LW", "UH_BA_SPEC", "UH_BA_NF"):
        monkeypatch.delenv(k, raising=False)
    if lw is not None:
        monkeypatch.setenv("UH_BA_LW", str(lw))
    if spec is not None:
        monkeypatch.setenv("UH_BA_SPEC", spec)
    got, again, ran_as = _run(hip_ctx, pr, n_iters)
    assert ran_as == form   # uh_ba_form: the persistent kernel ran, not a fallback
    monkeypatch.setenv("UH_BA_FORM", "legacy")
    chain, _, chain_as = _run(hip_ctx, pr, n_iters)
    assert chain_as == "chain"

    vs_chain = float(np.abs(got["state"] - chain["state"]).max())
    print(f"free {nfree} P {P} {ran_as}: iters {got['iters'].tolist()} | against the launch chain {vs_chain:.3g}")
    # the launch chain: the bars of test_ba.py between forms
    assert got["iters"].tolist() == chain["iters"].tolist()
    assert vs_chain < 1e-9
    _bad_flags_equal_up_to_the_boundary(got, chain)
    # a second run from the same snapshot: bit-identical
    for k in ("state", "poses", "points", "bad", "iters", "chi2"):
        np.testing.assert_array_equal(again[k], got[k])
