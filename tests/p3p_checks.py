"""What tests/test_p3p_branches_host.py (host build, numpy oracle) and tests/test_p3p_branches.py (device) assert of one implementation
against tests/golden/p3p_golden.npz, written once.  The fixture is loaded once and never written."""
from __future__ import annotations

import functools
import os

import numpy as np

import p3p_cases as K
import pnp_ransac_synth as S
from pnp_ransac_cases import TOL

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "p3p_golden.npz")
RODRIGUES_TOL = 1e-9        # |R(rvec) - R|, as tests/test_pnp_ransac_host.py::test_rodrigues_branches_against_the_oracle demands
RODRIGUES_SMALL = 1e-5      # p3p::kRodriguesSmall
EPS = 2.0 ** -53
ROOT_FACTOR, ROOT_FLOOR, SEPARATED = 1e3, 1e-12, 1e-4


@functools.lru_cache(maxsize=None)
def golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


@functools.lru_cache(maxsize=None)
def family(name):
    return K.family(name)


def rodrigues_branch(R):
    """'first_order', 'near_pi' or 'general': the branch of p3p::rodrigues a rotation matrix takes, and sin(theta)"""
    s = 0.5 * np.linalg.norm([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    c = 0.5 * (np.trace(R) - 1)
    return ("general" if s >= RODRIGUES_SMALL else ("first_order" if c > 0 else "near_pi")), s


def compare_family(name, solve):
    """solve(i) -> dict(n_solutions, Rt (n, 12), chosen, rvec_tvec (6) or None) of case i.  On every admitted case: the number of solutions
    equal, the pick equal where asserted, every solution's R, t within TOL, the chosen (rvec, tvec) giving back the reference's R within
    RODRIGUES_TOL and its t within TOL.  Returns the worst distance of a solution."""
    g, fam = golden(), family(name)
    worst = 0.0
    for i in np.nonzero(g[f"{name}_admitted"])[0]:
        got, n, where = solve(int(i)), int(g[f"{name}_n"][i]), f"{name}[{i}] seed {int(fam['seed'][i])} {fam['tag'][i]}"
        assert got["n_solutions"] == n, f"{where}: {got['n_solutions']} solutions, the reference has {n} at v = {g[f'{name}_v'][i][:n]}"
        if g[f"{name}_pick_asserted"][i]:
            assert got["chosen"] == int(g[f"{name}_pick"][i]), where
        for k in range(n):
            d = max(np.abs(got["Rt"][k, :9].reshape(3, 3) - g[f"{name}_R"][i, k]).max(), np.abs(got["Rt"][k, 9:] - g[f"{name}_t"][i, k]).max())
            assert d <= TOL, f"{where}: solution {k} is {d:.3g} from the reference"
            worst = max(worst, d)
        if n and got.get("rvec_tvec") is not None:
            c = got["chosen"]
            assert np.abs(S.rodrigues(got["rvec_tvec"][:3]) - g[f"{name}_R"][i, c]).max() <= RODRIGUES_TOL, where
            assert np.abs(got["rvec_tvec"][3:] - g[f"{name}_t"][i, c]).max() <= TOL, where
    return worst


def root_bounds(q):
    """per reference root of quartic q: (complex root, allowed |got - root|, 2^-53 cond, simple and real)"""
    g = golden()
    re, im, cond = g["quartic_re"][q], g["quartic_im"][q], g["quartic_cond"][q]
    out = []
    for k in range(4):
        if np.isnan(re[k]):
            continue
        r = complex(re[k], im[k])
        others = [complex(re[l], im[l]) for l in range(4) if l != k and not np.isnan(re[l])]
        sep = min([abs(r - o) / (1 + max(abs(r), abs(o))) for o in others], default=np.inf)
        out.append((r, max(ROOT_FACTOR * EPS * cond[k], ROOT_FLOOR * (1 + abs(r))), EPS * cond[k], im[k] == 0 and sep >= SEPARATED))
    return out


def compare_roots(roots, counts):
    """roots (n, 4) ascending with +inf for the absent ones, counts (n): an implementation's answer to K.quartics().  Every returned root
    lies within its bound of a reference root; every simple real reference root is returned; where all reference roots are SEPARATED
    apart the number of real roots is equal.  Returns {name: worst |error| / (2^-53 cond) over the matched roots}."""
    g, ratios = golden(), {}
    for q, (name, A) in enumerate(K.quartics()):
        assert np.array_equal(A, g["quartic_A"][q]), name
        ref = root_bounds(q)
        got = [float(x) for x in roots[q] if np.isfinite(x)]
        assert len(got) == int(counts[q]) and got == sorted(got), name
        worst = 0.0
        for x in got:
            d, bound, unit = min((abs(x - r), b, u) for r, b, u, _ in ref)
            assert d <= bound, f"{name}: returned root {x!r} is {d:.3g} from the nearest reference root, allowed {bound:.3g}"
            if 0 < unit < np.inf:
                worst = max(worst, d / unit)
        for r, b, _, simple in ref:
            if simple:
                assert any(abs(x - r) <= b for x in got), f"{name}: the simple root {r.real!r} is not returned (got {got})"
        if g["quartic_sep"][q] >= SEPARATED:
            assert len(got) == sum(1 for r, *_ in ref if r.imag == 0), name
        ratios[name] = worst
    return ratios
