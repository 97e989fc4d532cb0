"""Systems for the reduced-system solves (fp64 L D L^T without pivoting), one form at a time (tests/test_solve_forms.py drives them through
uh_ba_debug_solve / uh_posegraph_debug_solve; tests/test_solve_cases_host.py checks the claims made here on the CPU).  numpy and the standard
library only.

Family E — exact by construction.  L unit lower with entries in {-1, 0, 1}, D = +-2^k with |k| <= 3 and mixed signs, x integer in [-4, 4];
S = L D L^T and b = S x are formed in integers (everything is a multiple of 1/64: scaled by 64 it is an int64).  Every entry of S, of every
Schur complement, of L d and of z = D^-1 L^-1 b = L^T x, and every partial sum of the products l d l' in any order, is then a dyadic number
of a few bits: exact in double whatever the blocking, the order of accumulation or the contraction into FMAs.  The reciprocal of a power of
two is exact after one Newton step from any start that is good to half the bits.  So a solve must return x, L, D and z EQUAL to the
construction, and a dropped tile, a wrong ragged edge or a stale word is a gross integer error.

Family F — Family E with one D_k = 0: the zero pivot arises exactly at step k (the pivots before it are the D_j != 0), and the solve must
report failure.  Also non-finite entries, and -0.0 as a pivot.

Family R — random symmetric positive definite systems of a given 2-norm condition, rows and columns scaled by 10^+-3 in alternating groups of
three (rotations against translations); the measure is the normwise backward error against that of a plain unblocked numpy L D L^T.
"""
from __future__ import annotations

import functools
import math

import numpy as np

# form -> sizes: free keyframes (n = 6 nfree) for the bundle adjustment's forms 1-7, poses (n = 7 m) for the pose graph's ("7b")
SIZES = {
    1: (1, 2, 3, 4, 5, 6, 7, 8, 9, 10),   # backsolve_v2 has one instantiation per size
    2: (11, 12, 16),
    3: (1, 5, 10),
    4: (11, 17, 21),                      # 21: 127 rows, the two-rows-per-lane form's limit
    5: (22, 23, 27, 32),                  # 23: an odd count of block columns — an unpaired last panel
    6: (1, 2, 3, 33, 34, 47, 64),         # 64: 385 rows, one per thread of the workgroup
    7: (1, 10, 11, 21, 22, 65, 75),       # one partial panel; 64 + 2; two panels, ragged; seven panels
    "7b": (1, 9, 10, 18, 19, 28, 64, 65), # 63, 70, 126 / 133, 196, 448 = 7 x 64 (no ragged edge), 455
}
BLOCKED = (7, "7b")


def order_of(form, size) -> int:
    return 7 * size if form == "7b" else 6 * size


def cases(forms=None):
    """[(form, size)] of the table above"""
    return [(f, s) for f in (forms or SIZES) for s in SIZES[f]]


def case_id(c) -> str:
    return "form%s-%d" % c


# ---------------------------------------------------------------------------------------------------------------- Family E
def _seed(form, size, salt) -> int:
    return 1000003 * (8 if form == "7b" else int(form)) + 1009 * size + salt


def chord_rows(n: int):
    """the banded variant's long rows: [(row, (columns))], far below the band"""
    rows = [(n - 1, (1, n // 3)), (n - 3, (7, 70)), ((5 * n) // 8, (3, 66))]
    return [(r, tuple(c for c in cs if 0 <= c < r - 14)) for r, cs in rows if r > 30]


def unit_lower(n: int, rng, banded: bool):
    L = np.tril(rng.integers(-1, 2, (n, n)), -1).astype(np.int64)
    if banded:
        i, j = np.indices((n, n))
        L[i - j > 14] = 0
        for r, cs in chord_rows(n):
            for c in cs:
                L[r, c] = 1 if (r + c) % 2 else -1
    return L + np.eye(n, dtype=np.int64)


def exact_system(n: int, seed: int, banded: bool = False, zero_pivot: int | None = None, isolate: int | None = None):
    """dict(L int64 unit lower, D64 = 64 D int64, x int64, S64 = 64 S, b64 = 64 b) — exact integers.  zero_pivot: D_k = 0 there.  isolate: row
    and column k of L are cleared (the denormal case puts its own D_k there)."""
    rng = np.random.default_rng(seed)
    L = unit_lower(n, rng, banded)
    k = rng.integers(-3, 4, n)
    sign = np.where(rng.integers(0, 2, n) == 1, 1, -1)
    if n > 1:
        sign[0], sign[-1] = 1, -1   # (mixed signs whatever the draw)
    D64 = (sign * (2 ** (k + 6))).astype(np.int64)   # 64 * 2^k, 8 .. 512
    x = rng.integers(-4, 5, n).astype(np.int64)
    if zero_pivot is not None:
        D64[zero_pivot] = 0
    if isolate is not None:
        L[isolate, :isolate] = 0
        L[isolate + 1:, isolate] = 0
        x[isolate] = 3
    S64 = (L * D64) @ L.T
    b64 = S64 @ x
    return dict(L=L, D64=D64, x=x, S64=S64, b64=b64)


def as_double(e):
    """(S, b, L, D, x, z) of an exact system as float64 arrays (every conversion is exact: small dyadic numbers)"""
    S = e["S64"].astype(np.float64) / 64.0
    b = e["b64"].astype(np.float64) / 64.0
    z = (e["L"].T @ e["x"]).astype(np.float64)
    return S, b, e["L"].astype(np.float64), e["D64"].astype(np.float64) / 64.0, e["x"].astype(np.float64), z


@functools.lru_cache(maxsize=None)
def family_e(form, size, banded: bool = False):
    return exact_system(order_of(form, size), _seed(form, size, 7 if banded else 1), banded)


# ---------------------------------------------------------------------------------------------------------------- Family F
def zero_pivot_positions(form, size):
    """{name: k}: where Family F puts its zero pivot.  Block columns are six wide and the MFMA forms take them in pairs (0, 1), (2, 3), ...:
    row 6 is the first row of the second block column of the first pair, row 5 the last row of its first block column.  A position a
    system is too small for does not exist there."""
    n = order_of(form, size)
    pos = {"first": 0, "in_block": 6 * min(1, (n - 1) // 6) + 2, "pair_second_first": 6, "pair_first_last": 5, "last": n - 1}
    if form in BLOCKED:
        pos.update({"row63": 63, "row64": 64})
    return {k: v for k, v in pos.items() if 0 <= v < n}


@functools.lru_cache(maxsize=None)
def family_f(form, size, k: int):
    return exact_system(order_of(form, size), _seed(form, size, 3), zero_pivot=k)


def nonfinite_variants(S):
    """{name: S'} — one +Inf / NaN on the diagonal, one below it (in the lower triangle, which is what the solves read)"""
    n = len(S)
    kd, (i, j) = n // 2, (n - 1, max(0, n // 3 - 1))
    out = {}
    for name, v in (("inf", np.inf), ("nan", np.nan)):
        a = S.copy(); a[kd, kd] = v; out[name + "_diagonal"] = a
        if i > j:
            a = S.copy(); a[i, j] = v; a[j, i] = v; out[name + "_below"] = a
    return out


DENORMAL = 2.0 ** -1023


@functools.lru_cache(maxsize=None)
def denormal_case(form, size):
    """(S, b, x): Family E with row and column k of L cleared and D_k = 2^-1023, b_k = D_k x_k (x_k = 3: exact, a subnormal).  IEEE division
    gives 1 / D_k = 2^1023 and x_k = 3: finite and exact."""
    n = order_of(form, size)
    k = n // 2
    e = exact_system(n, _seed(form, size, 5), isolate=k)
    S, b, L, D, x, z = as_double(e)
    S[k, k] = DENORMAL
    b[k] = DENORMAL * 3.0
    return S, b, x, k


# ---------------------------------------------------------------------------------------------------------------- references
def ldlt_numpy(S, b):
    """Plain unblocked right-looking L D L^T in double with true division, products and sums rounded separately (numpy contracts nothing):
    (L unit lower, D, z = D^-1 L^-1 b, x, failed)."""
    n = len(b)
    A = np.array(S, np.float64)
    rhs = np.array(b, np.float64)
    L = np.eye(n)
    D = np.zeros(n)
    failed = False
    with np.errstate(all="ignore"):
        for k in range(n):
            d = A[k, k]
            D[k] = d
            if d == 0.0 or not np.isfinite(d):
                failed = True
            col = A[k + 1:, k].copy()
            l = col / d
            L[k + 1:, k] = l
            A[k + 1:, k + 1:] -= np.outer(l, col)
            rhs[k + 1:] -= l * rhs[k]
        z = rhs / D
        x = z.copy()
        for k in range(n - 1, 0, -1):
            x[:k] -= L[k, :k] * x[k]
    return L, D, z, x, failed


def _two_product(a, b):
    """Dekker: a * b = p + e exactly (Veltkamp splitting; no FMA needed), elementwise"""
    p = a * b
    c = 134217729.0   # 2^27 + 1
    ah = a * c; ah = ah - (ah - a); al = a - ah
    bh = b * c; bh = bh - (bh - b); bl = b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def backward_error(S, b, x, by_row: bool = False) -> float:
    """eta = ||b - S x||_inf / (||S||_inf ||x||_inf + ||b||_inf), the residual exact: every product split into two doubles, every row summed
    with math.fsum (correctly rounded).  by_row: max_i |r_i| / (|S| |x| + |b|)_i instead — the componentwise figure, which the scaling of
    rows and columns does not hide (reported beside eta, not asserted)."""
    p, e = _two_product(S, x[None, :])
    r = np.array([math.fsum([b[i]] + (-p[i]).tolist() + (-e[i]).tolist()) for i in range(len(b))])
    if by_row:
        return float((np.abs(r) / (np.abs(S) @ np.abs(x) + np.abs(b))).max())
    den = np.abs(S).sum(1).max() * np.abs(x).max() + np.abs(b).max()
    return float(np.abs(r).max() / den)


def factor_residual(S, L, D) -> float:
    """max |L D L^T - S| / max |S| over the lower triangle, evaluated in double (the same evaluation for the device and the reference)"""
    R = np.tril((L * D) @ L.T - S)
    return float(np.abs(R).max() / np.abs(S).max())


def diagonal_from(S, L):
    """the D that goes with a given unit lower L: d_j = S_jj - sum_t L_jt^2 d_t (for the forms that do not keep D)"""
    n = len(S)
    D = np.zeros(n)
    for j in range(n):
        D[j] = S[j, j] - np.dot(L[j, :j] * L[j, :j], D[:j])
    return D


# ---------------------------------------------------------------------------------------------------------------- Family R
R_CONDITIONS = (1e2, 1e6, 1e10)   # the targets: 2-norm condition before the rows and columns are scaled
R_SEED = 20260219
U = 2.0 ** -53
ETA_FACTOR = 8.0   # a different blocking order, FMA contraction and a 1-ulp reciprocal change roundings, not magnitudes


def spd_unscaled(n: int, cond: float, seed: int):
    """Q diag(sigma) Q^T + lambda I: sigma log-spaced over [1 / cond, 1], lambda = sigma_min / 2 (Levenberg's damping: cond falls by 1.5)"""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    sig = np.logspace(0.0, -math.log10(cond), n) if n > 1 else np.array([1.0])
    A = (Q * sig) @ Q.T + 0.5 * sig.min() * np.eye(n)
    return np.tril(A) + np.tril(A, -1).T


@functools.lru_cache(maxsize=None)
def family_r(form, size, cond: float):
    """dict(S, b, eta_ref, res_ref) — S exactly symmetric; the reference figures are those of ldlt_numpy on the same system"""
    n = order_of(form, size)
    seed = R_SEED + _seed(form, size, int(round(math.log10(cond))))
    A = spd_unscaled(n, cond, seed)
    s = np.where((np.arange(n) // 3) % 2 == 0, 1e3, 1e-3)
    S = A * s[:, None] * s[None, :]
    S = np.tril(S) + np.tril(S, -1).T
    x_true = np.random.default_rng(seed + 1).standard_normal(n) / s
    b = S @ x_true
    L, D, z, x, failed = ldlt_numpy(S, b)
    assert not failed
    # res_ref_derived: for the forms that do not keep D the residual is taken with the D that goes with their L (diagonal_from) — and so is
    # the reference's, like for like (a derived D moves the residual by roundings of its own, scaled by the rows' 1e+-3)
    return dict(S=S, b=b, unscaled=A, eta_ref=backward_error(S, b, x), res_ref=factor_residual(S, L, D),
                res_ref_derived=factor_residual(S, L, diagonal_from(S, L)), eta_rows_ref=backward_error(S, b, x, by_row=True))


# ---------------------------------------------------------------------------------------------------------------- exact elimination
def exact_factor(S64, b64):
    """Right-looking L D L^T of the bordered system [S; b^T] in exact integers (everything scaled by 64; an entry that leaves the multiples of
    1/64 raises).  dict(L int64, D64, z int64 (= D^-1 L^-1 b, an integer vector here), zero_at (first zero pivot or None: nothing behind
    it is computed), max64 (largest |entry| * 64 met anywhere), groups [(k0, {row group: nonempty})]).

    groups restates the 64-row grouping rule of csrc/dense_ldlt.hpp: panels start at multiples of 64; for the panel at k0 (columns k0 ..
    k0 + nb - 1) the rows behind it, border row n included, fall into groups r // 64, and a group is EMPTY when every entry of its rows in
    the panel's columns of the partly factorised matrix is zero.  The trailing update works on 64 x 64 tiles (row group, column group),
    column group <= row group, and leaves a tile out when either group is empty."""
    n = len(b64)
    A = np.zeros((n + 1, n + 1), np.int64)
    A[:n, :n] = np.tril(S64)
    A[n, :n] = b64
    L = np.eye(n, dtype=np.int64)
    D64 = np.zeros(n, np.int64)
    z = np.zeros(n, np.int64)
    out = dict(L=L, D64=D64, z=z, zero_at=None, max64=int(np.abs(A).max()), groups=[])
    for k in range(n):
        if k % 64 == 0:
            nb = min(64, n - k)
            nz = (A[k + nb:, k:k + nb] != 0).any(1)
            out["groups"].append((k, {int(g): bool(nz[np.arange(k + nb, n + 1) // 64 == g].any()) for g in np.unique(np.arange(k + nb, n + 1) // 64)}))
        d = int(A[k, k])
        D64[k] = d
        if d == 0:
            out["zero_at"] = k
            return out
        col = A[k + 1:, k].copy()          # 64 L d
        if (col % d).any():
            raise ArithmeticError("L left the integers at column %d" % k)
        l = col // d
        L[k + 1:n, k] = l[:-1]
        z[k] = l[-1]
        A[k + 1:, k + 1:n] -= np.tril(np.outer(l, col[:-1]))   # (lower triangle only; the border row has no column of its own)
        out["max64"] = max(out["max64"], int(np.abs(A[k + 1:, k + 1:]).max()), int(np.abs(l).max()) * 64)
    return out
