"""The three-point solver's branches ON THE DEVICE against the 60-digit reference of tests/golden/p3p_golden.npz (read only: mpmath is
not needed here).  Each family of tests/p3p_cases.py is one uh_pnp_ransac problem with n = 4 x cases, hypothesis i sampling the matches
4 i .. 4 i + 3; the debug hook runs every case (one wave, one root per lane: 1, 2, 3 and 4 live lanes, the rank bookkeeping of the hook and
of hyp_solve), and the same assertions as for the host build apply (tests/p3p_checks.py).  One solve() over all families: counts == -1
exactly where the reference has no solution, both root forms and two runs equal bit for bit.  The device's roots() on the quartics of
part B under the same condition-number bound as the host's.  Observed distances: profiles/p3p_branches.txt."""
import numpy as np
import pytest

import p3p_cases as K
import p3p_checks as PC
from pnp_ransac_cases import TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ransac(hip_ctx):
    from ucoslam_cv3_amd import PnPRansac

    r = PnPRansac(hip_ctx)
    yield r
    r.close()


@pytest.mark.parametrize("name", K.FAMILIES)
def test_device_hypotheses_against_the_reference(ransac, name):
    pr = K.problem(PC.family(name))

    def solve(i):
        d = ransac.debug_hypothesis(K.INTR, pr, i)
        return dict(n_solutions=d["n_solutions"], Rt=d["Rt"], chosen=d["chosen"], rvec_tvec=d["rvec_tvec"] if d["chosen"] >= 0 else None)

    worst = PC.compare_family(name, solve)
    print(f"{name}: device against the 60-digit reference, worst solution distance {worst:.3g}")
    assert worst <= TOL


def test_one_call_over_all_families(ransac):
    g = PC.golden()
    prs = [K.problem(PC.family(name)) for name in K.FAMILIES]
    one = ransac.solve(K.INTR, prs)
    for name, r in zip(K.FAMILIES, one):
        adm = g[f"{name}_admitted"]
        assert np.array_equal((r["counts"] == -1)[adm], (g[f"{name}_n"] == 0)[adm]), name
    ransac.set_form(True)
    try:
        two = ransac.solve(K.INTR, prs)
    finally:
        ransac.set_form(False)
    three = ransac.solve(K.INTR, prs)
    for a, b, c in zip(one, two, three):
        assert (a["ok"], a["n_inliers"], a["best_iter"]) == (b["ok"], b["n_inliers"], b["best_iter"]) == (c["ok"], c["n_inliers"], c["best_iter"])
        for k in ("rt6", "pose", "inliers", "counts"):
            assert a[k].tobytes() == b[k].tobytes() == c[k].tobytes(), k


def test_device_roots_against_the_reference(ransac):
    roots, counts = ransac.debug_roots(np.stack([A for _, A in K.quartics()]))
    for n, r in PC.compare_roots(roots, counts).items():
        print(f"{n}: device roots(), worst error {r:.3g} x 2^-53 cond")
