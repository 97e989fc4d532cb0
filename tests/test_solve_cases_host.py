"""The generators of tests/solve_cases.py, checked alone on the CPU: what the GPU tests of the solve forms (test_solve_forms.py) take for
granted about their inputs and references is asserted here in exact arithmetic."""
from fractions import Fraction

import numpy as np
import pytest

import solve_cases as sc

ALL = sc.cases()
BLOCKED = sc.cases(sc.BLOCKED)


def _variants(form):
    return (False, True) if form in sc.BLOCKED else (False,)


@pytest.mark.parametrize("case", ALL, ids=sc.case_id)
def test_family_e_is_exact_in_double(case):
    """Elimination in exact integers (everything scaled by 64) gives the construction back; every entry met on the way is a multiple of
    1/64 below 2^50 — representable — and so is every partial sum of the products l d l', whatever its order."""
    for banded in _variants(case[0]):
        e = sc.family_e(*case, banded)
        f = sc.exact_factor(e["S64"], e["b64"])
        assert f["zero_at"] is None
        assert np.array_equal(f["L"], e["L"]) and np.array_equal(f["D64"], e["D64"]) and np.array_equal(f["z"], e["L"].T @ e["x"])
        assert f["max64"] < 64 * 2 ** 50
        absum = (np.abs(e["L"]) * np.abs(e["D64"])) @ np.abs(e["L"]).T   # 64 sum_t |l_it d_t l_jt|: bounds every partial sum of a Schur complement
        assert absum.max() + np.abs(e["S64"]).max() < 2 ** 53
        assert (np.abs(e["L"].T) @ np.abs(e["x"])).max() < 2 ** 53 and np.abs(e["b64"]).max() < 2 ** 53
        assert set(np.unique(np.abs(e["D64"]))) <= {8, 16, 32, 64, 128, 256, 512} and (e["D64"] > 0).any() and (e["D64"] < 0).any()
        assert np.abs(e["x"]).max() <= 4 and set(np.unique(e["L"])) <= {-1, 0, 1}


@pytest.mark.parametrize("case", ALL, ids=sc.case_id)
def test_numpy_ldlt_reproduces_family_e_bit_for_bit(case):
    for banded in _variants(case[0]):
        S, b, L, D, x, z = sc.as_double(sc.family_e(*case, banded))
        L2, D2, z2, x2, failed = sc.ldlt_numpy(S, b)
        assert not failed
        for got, want in ((L2, L), (D2, D), (z2, z), (x2, x)):
            assert np.array_equal(got, want)
        assert sc.backward_error(S, b, x2) == 0.0 and sc.factor_residual(S, L2, D2) == 0.0


@pytest.mark.parametrize("case", ALL, ids=sc.case_id)
def test_family_f_zero_pivot_arises_at_k_and_not_before(case):
    pos = sc.zero_pivot_positions(*case)
    assert {"first", "last"} <= set(pos)
    n = sc.order_of(*case)
    if n >= 12:
        assert {"in_block", "pair_second_first", "pair_first_last"} <= set(pos) and pos["in_block"] % 6 not in (0, 5)
    if case[0] in sc.BLOCKED and n > 64:
        assert pos["row63"] == 63 and pos["row64"] == 64
    for k in pos.values():
        e = sc.family_f(*case, k)
        f = sc.exact_factor(e["S64"], e["b64"])
        assert f["zero_at"] == k and (f["D64"][:k] != 0).all()
        S, b = sc.as_double(e)[:2]
        assert sc.ldlt_numpy(S, b)[4]
        for name, Sv in sc.nonfinite_variants(sc.as_double(sc.family_e(*case))[0]).items():
            assert sc.ldlt_numpy(Sv, b)[4], name


@pytest.mark.parametrize("case", [c for c in BLOCKED if sc.order_of(*c) >= 192], ids=sc.case_id)
def test_banded_pattern_has_the_empty_groups_the_skip_logic_is_about(case):
    """At least one panel has an empty 64-row group strictly between two non-empty ones, and at least one update tile has an empty row group
    together with a non-empty column group (column group <= row group)."""
    e = sc.family_e(*case, True)
    groups = sc.exact_factor(e["S64"], e["b64"])["groups"]
    between = tile = False
    for k0, g in groups:
        ids = sorted(g)
        full = [i for i in ids if g[i]]
        between |= any(not g[i] and full and min(full) < i < max(full) for i in ids)
        tile |= any(not g[r] and g[c] for r in ids for c in ids if c <= r)
    assert between and tile
    dense = sc.exact_factor(*[sc.family_e(*case)[k] for k in ("S64", "b64")])["groups"]
    assert all(all(g.values()) for _, g in dense)   # (the dense variant skips nothing)


@pytest.mark.parametrize("case", ALL, ids=sc.case_id)
def test_denormal_case_is_finite_and_exact_under_ieee_division(case):
    S, b, x, k = sc.denormal_case(*case)
    assert S[k, k] == 2.0 ** -1023 and b[k] == 3 * 2.0 ** -1023 and not S[k, :k].any() and not S[k + 1:, k].any()
    L, D, z, x2, failed = sc.ldlt_numpy(S, b)
    assert not failed and np.array_equal(x2, x) and x[k] == 3 and D[k] == 2.0 ** -1023


@pytest.mark.parametrize("case", ALL, ids=sc.case_id)
def test_family_r_conditions_and_reference_error(case):
    for cond in sc.R_CONDITIONS:
        r = sc.family_r(*case, cond)
        if sc.order_of(*case) > 1:
            got = np.linalg.cond(r["unscaled"])
            assert cond / 3 <= got <= cond * 3, (cond, got)
        assert np.array_equal(r["S"], r["S"].T)
        assert r["eta_ref"] < 100 * sc.U, (cond, r["eta_ref"])   # (so that 8 x eta_ref is a bound worth the name)


def test_backward_error_is_the_exact_residual():
    r = sc.family_r(6, 2, 1e6)
    S, b = r["S"], r["b"]
    x = sc.ldlt_numpy(S, b)[3]
    res = [Fraction(float(b[i])) - sum(Fraction(float(S[i, j])) * Fraction(float(x[j])) for j in range(len(b))) for i in range(len(b))]
    den = Fraction(float(np.abs(S).sum(1).max())) * Fraction(float(np.abs(x).max())) + Fraction(float(np.abs(b).max()))
    exact = float(max(abs(v) for v in res) / den)
    assert abs(sc.backward_error(S, b, x) - exact) <= 4 * sc.U * exact
