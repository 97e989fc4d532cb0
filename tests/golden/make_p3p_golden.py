"""Generates tests/golden/p3p_golden.npz: the three-point problem of csrc/p3p_math.hpp in 60-digit arithmetic (mpmath), and the roots of
the quartics of tests/p3p_cases.py by mpmath.polyroots.  No OpenCV exists to compare the solver with; this pins it to its mathematical
contract (include/ucoslam_hip.h): every real solution with positive point distances, numbered in ascending s3 / s1, the one with the
smallest reprojection error of the fourth point, the lowest index on ties.

Per case (float32 inputs, taken exactly): the unit bearings and the cosine-rule system of Grunert; the quartic in v = s3 / s1 with its
coefficients formed in 60 digits; its roots by polyroots; per real root with v > 0 and u = s2 / s1 > 0 the three distances, polished by
Newton on the three cosine-rule equations; the pose NOT by the kernel's two orthonormal frames but by an orthogonal Procrustes solve
(SVD of the 3 x 3 correlation of the two congruent triangles, their normals added as a third pair).  Every solution is checked on its
own to 1e-30: R'R = I, det R = 1, every sample point on its bearing at its distance.

Admission (by the reference alone, stored as `<family>_admitted`):
  the smallest relative gap between two real roots and the smallest |Im| / (1 + |Re|) of a complex root are >= 1e-4;
  the smallest v and u over the solutions are >= 1e-6.
`<family>_pick_asserted`: the two smallest fourth-point errors differ by more than 1e-6 relative.
No family may lose more than 10 % of its cases; a rejected seed of `a4` or `rot` is replaced in p3p_cases.SEEDS (FIRST_CHOICE keeps it).

  python tests/golden/make_p3p_golden.py            writes the fixture
  python tests/golden/make_p3p_golden.py --check    regenerates and compares with the committed file"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
import oracle_lib  # noqa: E402
import p3p_cases  # noqa: E402

GOLDEN = os.path.join(HERE, "p3p_golden.npz")
DPS = 60
SELF_CHECK = 1e-30
GAP, MIN_VU, PICK_GAP, MAX_LOSS = 1e-4, 1e-6, 1e-6, 0.10
REAL = 1e-40       # a root of the 60-digit solve counts as real below this |Im| / (1 + |Re|)


def mpmath_available():
    """None, or why the generator cannot run here"""
    try:
        import mpmath  # noqa: F401
    except Exception as e:   # noqa: BLE001
        return f"mpmath does not import ({e})"
    return None


def input_digest(fam):
    return oracle_lib.digest(fam["P"], fam["px"], np.asarray(p3p_cases.INTR, np.float32))


def quartic_digest(qs):
    return oracle_lib.digest(*[c for _, c in qs])


def _polymul(a, b):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] = out[i + j] + x * y
    return out


def solve_case(mp, intr, P, px):
    """One hypothesis in mp arithmetic -> dict of float64 arrays (padded to four solutions)."""
    mpf, mat = mp.mpf, mp.matrix
    fx, fy, cx, cy = [mpf(float(v)) for v in intr]
    X = [mat([mpf(float(v)) for v in P[i]]) for i in range(4)]
    xn = [((mpf(float(px[i, 0])) - cx) / fx, (mpf(float(px[i, 1])) - cy) / fy) for i in range(4)]
    j = []
    for i in range(3):
        b = mat([xn[i][0], xn[i][1], mpf(1)])
        j.append(b / mp.norm(b))
    dot = lambda a, b: sum(a[k] * b[k] for k in range(3))   # noqa: E731
    a2, b2, c2 = dot(X[2] - X[1], X[2] - X[1]), dot(X[2] - X[0], X[2] - X[0]), dot(X[1] - X[0], X[1] - X[0])
    ca, cb, cg = dot(j[1], j[2]), dot(j[0], j[2]), dot(j[0], j[1])
    k, q = (a2 - c2) / b2, c2 / b2
    # ascending powers of v
    N, D, Wp = [k + 1, -2 * k * cb, k - 1], [2 * cg, -2 * ca], [1 - q, 2 * q * cb, -q]
    NN, DDW, ND = _polymul(N, N), _polymul(_polymul(D, D), Wp), _polymul(N, D) + [0]
    A = [NN[i] + DDW[i] - 2 * cg * ND[i] for i in range(5)]
    amax = max(abs(c) for c in A)
    hi = list(reversed(A))
    while hi and hi[0] == 0:
        hi.pop(0)
    rts = mp.polyroots(hi, maxsteps=500, extraprec=4 * mp.mp.prec) if len(hi) > 1 else []
    real = sorted([mp.re(r) for r in rts if abs(mp.im(r)) <= REAL * (1 + abs(mp.re(r)))])
    cplx = [r for r in rts if abs(mp.im(r)) > REAL * (1 + abs(mp.re(r)))]
    gap = min([abs(real[a] - real[b]) / (1 + max(abs(real[a]), abs(real[b]))) for a in range(len(real)) for b in range(a)], default=mp.inf)
    imag = min([abs(mp.im(r)) / (1 + abs(mp.re(r))) for r in cplx], default=mp.inf)
    out = dict(n=0, R=np.zeros((4, 3, 3)), t=np.zeros((4, 3)), s=np.zeros((4, 3)), v=np.full(4, np.inf), err4=np.full(4, np.inf), pick=-1, pick_asserted=True,
               gap=float(gap), imag=float(imag), min_vu=np.inf, A=np.array([float(c / amax) for c in A]), n_real=len(real), check=0.0)
    errs, min_vu, worst = [], mp.inf, mpf(0)
    for v in real:
        Dv = D[0] + D[1] * v
        if not v > 0 or Dv == 0:
            continue
        u = (N[0] + N[1] * v + N[2] * v * v) / Dv
        if not u > 0:
            continue
        s1 = mp.sqrt(b2 / (1 + v * v - 2 * v * cb))
        s = mat([s1, u * s1, v * s1])
        for _ in range(3):   # Newton on the three cosine-rule equations themselves
            f = mat([s[1] ** 2 + s[2] ** 2 - 2 * s[1] * s[2] * ca - a2, s[0] ** 2 + s[2] ** 2 - 2 * s[0] * s[2] * cb - b2,
                     s[0] ** 2 + s[1] ** 2 - 2 * s[0] * s[1] * cg - c2])
            J = mat([[0, 2 * (s[1] - s[2] * ca), 2 * (s[2] - s[1] * ca)], [2 * (s[0] - s[2] * cb), 0, 2 * (s[2] - s[0] * cb)],
                     [2 * (s[0] - s[1] * cg), 2 * (s[1] - s[0] * cg), 0]])
            s = s - mp.lu_solve(J, f)
        Q = [s[i] * j[i] for i in range(3)]
        # orthogonal Procrustes between the two congruent triangles (their normals as a third pair make the correlation full rank)
        def pairs(T):
            e1, e2 = T[1] - T[0], T[2] - T[0]
            return [e1, e2, mat([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]])]
        Hm = mp.zeros(3, 3)
        for aw, bc in zip(pairs(X[:3]), pairs(Q)):
            Hm += bc * aw.T
        U, _, V = mp.svd_r(Hm)
        R = U * V
        if mp.det(R) < 0:
            R = U * mp.diag([1, 1, -1]) * V
        Pm, Qm = (X[0] + X[1] + X[2]) / 3, (Q[0] + Q[1] + Q[2]) / 3
        t = Qm - R * Pm
        # the solution on its own
        chk = max(mp.norm(R.T * R - mp.eye(3), p=mp.inf), abs(mp.det(R) - 1), *[mp.norm(R * X[i] + t - s[i] * j[i], p=mp.inf) for i in range(3)])
        worst = max(worst, chk)
        assert chk <= SELF_CHECK, f"self-check {mp.nstr(chk, 5)}"
        Xc = R * X[3] + t
        e = (Xc[0] / Xc[2] - xn[3][0]) ** 2 + (Xc[1] / Xc[2] - xn[3][1]) ** 2
        i = out["n"]
        out["R"][i] = np.array([[float(R[a, b]) for b in range(3)] for a in range(3)])
        out["t"][i] = [float(t[a]) for a in range(3)]
        out["s"][i] = [float(s[a]) for a in range(3)]
        out["v"][i] = float(s[2] / s[0])
        out["err4"][i] = float(e)
        errs.append(e)
        min_vu = min(min_vu, s[2] / s[0], s[1] / s[0])
        out["n"] += 1
    if errs:
        order = sorted(range(len(errs)), key=lambda i: (errs[i], i))
        out["pick"] = order[0]
        if len(errs) > 1:
            e0, e1 = errs[order[0]], errs[order[1]]
            out["pick_asserted"] = bool(e1 - e0 > PICK_GAP * e1)
    out["min_vu"], out["check"] = float(min_vu), float(worst)
    out["admitted"] = bool(out["gap"] >= GAP and out["imag"] >= GAP and out["min_vu"] >= MIN_VU)
    return out


KEYS = ("n", "R", "t", "s", "v", "err4", "pick", "pick_asserted", "gap", "imag", "min_vu", "A", "n_real", "check", "admitted")


def solve_quartic(mp, c):
    """roots (re, im), condition numbers sum |A_i| |r|^i / |P'(r)| and the smallest relative separation of two roots, padded to four"""
    A = [mp.mpf(float(x)) for x in c]
    hi = list(reversed(A))
    while hi and hi[0] == 0:
        hi.pop(0)
    rts = mp.polyroots(hi, maxsteps=2000, extraprec=40 * mp.mp.prec)
    rts = sorted(rts, key=lambda r: (mp.re(r), mp.im(r)))
    re, im, cond = np.full(4, np.nan), np.full(4, np.nan), np.full(4, np.nan)
    for i, r in enumerate(rts):
        dP = sum(k * A[k] * r ** (k - 1) for k in range(1, 5))
        re[i], im[i] = float(mp.re(r)), (0.0 if abs(mp.im(r)) <= REAL * (1 + abs(mp.re(r))) else float(mp.im(r)))
        cond[i] = float(sum(abs(A[k]) * abs(r) ** k for k in range(5)) / abs(dP)) if dP != 0 else np.inf
    sep = min([float(abs(rts[a] - rts[b]) / (1 + max(abs(rts[a]), abs(rts[b])))) for a in range(len(rts)) for b in range(a)], default=np.inf)
    return re, im, cond, sep


def generate(verbose=True):
    import mpmath as mp

    mp.mp.dps = DPS
    save = {}
    for name in p3p_cases.FAMILIES:
        fam = p3p_cases.family(name)
        outs = [solve_case(mp, p3p_cases.INTR, fam["P"][i], fam["px"][i]) for i in range(len(fam["P"]))]
        for k in KEYS:
            save[f"{name}_{k}"] = np.array([o[k] for o in outs])
        save[f"{name}_in_digest"] = input_digest(fam)
        adm = save[f"{name}_admitted"]
        if verbose:
            print(f"{name}: {len(outs)} cases, {int(adm.sum())} admitted, solutions {np.bincount(save[f'{name}_n'], minlength=5).tolist()}, "
                  f"pick asserted {int(save[f'{name}_pick_asserted'].sum())}, worst self-check {save[f'{name}_check'].max():.2e}, "
                  f"rejected {[(int(fam['seed'][i]), str(fam['tag'][i])) for i in np.nonzero(~adm)[0]]}")
        assert (~adm).sum() <= MAX_LOSS * len(outs), f"{name}: more than 10 % of the cases rejected"
    qs = p3p_cases.quartics()
    sol = [solve_quartic(mp, c) for _, c in qs]
    save["quartic_A"] = np.stack([c for _, c in qs])
    save["quartic_re"], save["quartic_im"], save["quartic_cond"] = [np.stack([s[i] for s in sol]) for i in range(3)]
    save["quartic_sep"] = np.array([s[3] for s in sol])
    save["quartic_in_digest"] = quartic_digest(qs)
    return save


def check():
    """Digests, counts, picks and flags exactly; floating point to 1e-13 (1 + |v|): the 60-digit results are rounded once, and only
    the case inputs (numpy's sin / cos) could differ between machines, which the digests would show."""
    old, new = np.load(GOLDEN), generate(verbose=False)
    assert sorted(old.files) == sorted(new), "the fixture's keys differ"
    for k in old.files:
        a, b = old[k], np.asarray(new[k])
        if a.dtype.kind in "iub":
            assert np.array_equal(a, b), k
        else:
            fin = np.isfinite(a)
            assert np.array_equal(fin, np.isfinite(b)) and np.array_equal(a[~fin], b[~fin], equal_nan=True), k
            assert (np.abs(a[fin] - b[fin]) <= 1e-13 * (1 + np.abs(a[fin]))).all(), k
    print("p3p_golden.npz reproduced")


if __name__ == "__main__":
    why = mpmath_available()
    assert why is None, why
    if len(sys.argv) > 1 and sys.argv[1] == "--check":
        check()
    else:
        np.savez_compressed(GOLDEN, **generate())
        print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
