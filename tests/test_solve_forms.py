"""Every reduced-system solve form (fp64 L D L^T without pivoting) on its own, through uh_ba_debug_solve / uh_posegraph_debug_solve — the hooks
run the production device functions and launches on a system the test gives (csrc/solve_debug.hpp).

  Family E  exact by construction: x, L, D (where the form keeps it), z and failed = 0 must EQUAL the construction, bit for bit.
  Family F  a zero pivot that arises exactly on the device, +-Inf / NaN entries, -0.0 as a pivot: failed = 1 (and x = 0 in the bundle
            adjustment's forms); one denormal pivot, where IEEE division gives a finite exact answer.
  Family R  conditions 1e2 / 1e6 / 1e10 with rows and columns scaled by 1e+-3: backward error and factor residual within 8 x those of a plain
            unblocked numpy L D L^T (never below the unit roundoff 2^-53).
The cases, their sizes and the references are tests/solve_cases.py's; tests/test_solve_cases_host.py checks them on the CPU.
"""
import numpy as np
import pytest

import solve_cases as sc

pytestmark = pytest.mark.gpu
ALL = sc.cases()


class _Solver:
    """one uh_ba / uh_posegraph handle behind a common call"""

    def __init__(self, ctx, form):
        from ucoslam_cv3_amd.ba import GlobalOptimizer
        from ucoslam_cv3_amd.posegraph import PoseGraph

        self.form = form
        self.h = PoseGraph(ctx) if form == "7b" else GlobalOptimizer(ctx)

    def __call__(self, S, b):
        return self.h.debug_solve(S, b) if self.form == "7b" else self.h.debug_solve(self.form, S, b)

    def close(self):
        self.h.close()


@pytest.fixture(scope="module")
def solvers(hip_ctx):
    made = {f: _Solver(hip_ctx, f) for f in sc.SIZES}
    yield made
    for s in made.values():
        s.close()


def _variants(form):
    return (False, True) if form in sc.BLOCKED else (False,)


def _assert_equals_construction(out, L, D, x, z, what, blocked=False):
    assert out["failed"] == 0, what
    z0 = ((len(x) - 1) // 64) * 64 if blocked else 0   # (the blocked forms substitute in the row that held z: the last panel's part is left)
    for name, got, want in (("x", out["x"], x), ("z", out["z"][z0:], z[z0:]), ("L", out["L"], L), ("D", out["D"], D)):
        if got is None:   # (a form that does not keep D)
            continue
        bad = np.argwhere(got != want)
        assert len(bad) == 0, "%s: %s differs from the construction at %d places, first %s: %r != %r" % (
            what, name, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("case", ALL, ids=sc.case_id)
def test_family_e_equals_the_construction(solvers, case):
    form, size = case
    for banded in _variants(form):
        S, b, L, D, x, z = sc.as_double(sc.family_e(form, size, banded))
        _assert_equals_construction(solvers[form](S, b), L, D, x, z, "%s%s" % (sc.case_id(case), " banded" if banded else ""), form in sc.BLOCKED)


@pytest.mark.parametrize("case", ALL, ids=sc.case_id)
def test_family_f_reports_failure(solvers, case):
    form, size = case
    solve = solvers[form]
    n = sc.order_of(form, size)

    def must_fail(S, b, what):
        out = solve(S, b)
        assert out["failed"] == 1, "%s %s: the solve did not report failure" % (sc.case_id(case), what)
        if form != "7b":
            assert not out["x"].any(), "%s %s: x is not zero behind a failed solve" % (sc.case_id(case), what)

    for name, k in sc.zero_pivot_positions(form, size).items():
        S, b = sc.as_double(sc.family_f(form, size, k))[:2]
        must_fail(S, b, "zero pivot %s (row %d)" % (name, k))
    S, b = sc.as_double(sc.family_f(form, size, 0))[:2]
    S[0, 0] = -0.0
    must_fail(S, b, "-0.0 as the first pivot")
    S0, b0, L, D, x, z = sc.as_double(sc.family_e(form, size))
    for name, Sv in sc.nonfinite_variants(S0).items():
        must_fail(Sv, b0, name)
    # ... and with a finite non-zero pivot everywhere the same handle solves again (nothing of the failures is left behind)
    _assert_equals_construction(solve(S0, b0), L, D, x, z, sc.case_id(case) + " after the failures", form in sc.BLOCKED)
    assert n == len(b0)


@pytest.mark.parametrize("case", ALL, ids=sc.case_id)
def test_denormal_pivot(solvers, case):
    """D_k = 2^-1023 on a row and column of its own: IEEE division gives 1 / D_k = 2^1023 and x_k = 3 exactly, failed = 0."""
    form, size = case
    S, b, x, k = sc.denormal_case(form, size)
    out = solvers[form](S, b)
    print("SOLVE_DENORMAL form=%s size=%d failed=%d x_k=%r (reference 3.0) x_equal=%s" % (form, size, out["failed"], out["x"][k], np.array_equal(out["x"], x)))
    assert np.array_equal(out["x"], x), "x differs from the IEEE result: x_k = %r" % out["x"][k]
    assert out["failed"] == 0


@pytest.mark.parametrize("cond", sc.R_CONDITIONS, ids=lambda c: "cond%.0e" % c)
@pytest.mark.parametrize("case", ALL, ids=sc.case_id)
def test_family_r_rounding_quality(solvers, case, cond):
    form, size = case
    r = sc.family_r(form, size, cond)
    S, b = r["S"], r["b"]
    out = solvers[form](S, b)
    assert out["failed"] == 0
    eta = sc.backward_error(S, b, out["x"])
    # (a form that does not keep D: the residual with the D that goes with its L, against the reference's taken the same way)
    D, res_ref = (out["D"], r["res_ref"]) if out["D"] is not None else (sc.diagonal_from(S, out["L"]), r["res_ref_derived"])
    res = sc.factor_residual(S, out["L"], D)
    print("SOLVE_R form=%s size=%d n=%d cond=%.0e eta=%.3e eta_ref=%.3e res=%.3e res_ref=%.3e eta_rows=%.3e eta_rows_ref=%.3e" % (
        form, size, len(b), cond, eta, r["eta_ref"], res, res_ref, sc.backward_error(S, b, out["x"], by_row=True), r["eta_rows_ref"]))
    assert eta <= sc.ETA_FACTOR * max(r["eta_ref"], sc.U), (eta, r["eta_ref"])
    assert res <= sc.ETA_FACTOR * max(res_ref, sc.U), (res, res_ref)


@pytest.mark.parametrize("form", list(sc.SIZES), ids=lambda f: "form%s" % f)
def test_repeatable_and_nothing_stale(hip_ctx, solvers, form):
    """Two calls on one handle are bit-identical, and a small system behind a large one on the same handle equals the small one on a fresh
    handle (stale LDS or HBM words beyond n)."""
    small, large = min(sc.SIZES[form]), max(sc.SIZES[form])
    rl, rs = sc.family_r(form, large, 1e6), sc.family_r(form, small, 1e6)
    solve = solvers[form]
    a, a2 = solve(rl["S"], rl["b"]), solve(rl["S"], rl["b"])
    # (x and the factor, not the raw matrix: the word the MFMA forms redirect their absent tile elements to takes whatever lane stores last)
    for k in ("x", "L", "D", "z"):
        assert (a[k] is None and a2[k] is None) or a[k].tobytes() == a2[k].tobytes(), "two calls differ in " + k
    assert a["failed"] == a2["failed"] == 0
    after = solve(rs["S"], rs["b"])
    fresh_solver = _Solver(hip_ctx, form)
    try:
        fresh = fresh_solver(rs["S"], rs["b"])
    finally:
        fresh_solver.close()
    for k in ("x", "L", "z"):
        assert after[k].tobytes() == fresh[k].tobytes(), "small after large differs from small on a fresh handle in " + k
    assert after["failed"] == fresh["failed"] == 0


def test_a_form_refuses_a_size_it_cannot_hold(hip_ctx, solvers):
    import ctypes as C

    from ucoslam_cv3_amd._lib import lib, np_ptr
    from ucoslam_cv3_amd.ba import SOLVE_FORMS

    h = solvers[1].h._h
    for form, (lo, hi, _) in SOLVE_FORMS.items():
        for nfree in (lo - 1, hi + 1):
            n = 6 * max(nfree, 1)
            S, b, x, failed = np.eye(n), np.ones(n), np.full(n, 7.0), C.c_int(-5)
            rc = lib().uh_ba_debug_solve(h, form, nfree, np_ptr(S), np_ptr(b), np_ptr(x), None, C.byref(failed))
            assert rc == -1 and failed.value == -5 and (x == 7.0).all(), (form, nfree)   # UH_EINVAL, nothing written
    for form in (0, 8):
        S, b, x, failed = np.eye(6), np.ones(6), np.zeros(6), C.c_int(-5)
        assert lib().uh_ba_debug_solve(h, form, 1, np_ptr(S), np_ptr(b), np_ptr(x), None, C.byref(failed)) == -1
