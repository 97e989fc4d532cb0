"""The map initialiser, the part that needs no GPU: a stand-alone host build of csrc/mapinit_math.hpp against the numpy oracle
(tests/mapinit_oracle.py), uh_mapinit_samples against the oracle's draws, the whole uh_mapinit_run_host against the oracle on every
scene of tests/mapinit_cases.py, and the scenes' own conditions on the oracle alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mapinit_cases as MC
import mapinit_oracle as O
from mapinit_checks import assert_agrees_with_oracle, assert_planted_non_finite
from ucoslam_cv3_amd import mapinit as MI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELPER = os.path.join(ROOT, "tests", "host_helpers", "mapinit_math_host.cpp")
F = np.float32
FP, DP = C.POINTER(C.c_float), C.POINTER(C.c_double)


def fp(a):
    return a.ctypes.data_as(FP)


def dp(a):
    return a.ctypes.data_as(DP)


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("mapinit") / "libmapinit_math_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", "-o", so, HELPER])
    L = C.CDLL(so)
    L.mi_det3.restype = C.c_float
    return L


def sample_systems(name, count):
    """the float32 8-point systems of the first `count` samples of a scene, as the oracle builds them"""
    sc, r = MC.scene(name), MC.oracle(name)
    kp1, kp2, m = sc["kp1"], sc["kp2"], sc["matches"]
    mx1, my1, sx1, sy1, _ = O.normalise(kp1)
    mx2, my2, sx2, sy2, _ = O.normalise(kp2)
    n1 = np.stack([(kp1[m[:, 0], 0] - mx1) * sx1, (kp1[m[:, 0], 1] - my1) * sy1], 1)
    n2 = np.stack([(kp2[m[:, 1], 0] - mx2) * sx2, (kp2[m[:, 1], 1] - my2) * sy2], 1)
    for s in r["samples"][:count]:
        yield O.system_h(n1[s], n2[s]), O.system_f(n1[s], n2[s])


def test_null_vectors_match_lapack(host_lib):
    """Both null vectors against LAPACK under the same sign rule.  Bar: a singular vector moves by (perturbation of the matrix) /
    (gap to the neighbouring singular value); both solvers perturb the matrix by a few times the double rounding 1.1e-16 relative to
    sigma_1.  So the bar is 1e-14 * sigma_1 / (sigma_8 - sigma_9), about a hundred roundings."""
    worst = 0.0
    for name in ("general_1000", "plane_1000"):
        for Ah, Af in sample_systems(name, 60):
            for A in (Ah, Af):
                x = np.zeros(9)
                host_lib.mi_null_vector(fp(np.ascontiguousarray(A, F)), len(A), dp(x))
                ref, cond = O.null_vector(A)
                w = np.linalg.svd(A.astype(np.float64), compute_uv=False)
                gap = w[7] - (w[8] if len(w) > 8 else 0.0)
                err = np.abs(x - ref).max()
                worst = max(worst, err * gap / w[0])
                assert abs(np.linalg.norm(x) - 1) < 1e-14
                assert err <= 1e-14 * w[0] / gap, (name, err, w[0] / gap)
    print(f"worst null-vector error times gap / sigma_1: {worst:.3e}")


def test_svd3_rank2_inverse_determinant(host_lib):
    rng = np.random.default_rng(5)
    for k in range(200):
        A = rng.normal(size=(3, 3)).astype(F)
        if k % 4 == 1:
            A[:, 2] = A[:, 0] * F(0.5) + A[:, 1]          # rank 2 up to float rounding
        if k % 4 == 2:
            A = (np.diag([1.0, 1.0 + 1e-6 * (k % 7), 0.3]) @ A.astype(np.float64)).astype(F)
        U, w, V = np.zeros(9), np.zeros(3), np.zeros(9)
        host_lib.mi_svd3(fp(A), dp(U), dp(w), dp(V))
        U, V = U.reshape(3, 3), V.reshape(3, 3)
        Uo, wo, Vto = O.svd3(A)
        assert np.abs(w - wo).max() <= 1e-14 * wo[0]
        tiny = not wo[2] > 1e-10 * wo[0]   # the sign rule then takes u3 from u1 x u2: its term sigma_3 u3 v3^T may come back with the other sign
        assert np.abs((U * w) @ V.T - A.astype(np.float64)).max() <= 1e-14 * wo[0] + (2 * wo[2] if tiny else 0.0)
        assert np.abs(U.T @ U - np.eye(3)).max() < 1e-9 and np.abs(V.T @ V - np.eye(3)).max() < 1e-13
        gap = min(wo[0] - wo[1], wo[1] - wo[2])
        if gap > 1e-3 * wo[0] and wo[2] > 1e-6 * wo[0]:   # separated singular values: the vectors themselves are determined
            assert np.abs(V - Vto.T).max() < 1e-10 and np.abs(U - Uo).max() < 1e-8
        Fn = np.zeros(9, F)
        host_lib.mi_rank2(fp(A), fp(Fn))
        ref = O.rank2(A)
        assert np.abs(Fn.reshape(3, 3) - ref).max() <= 4 * np.finfo(F).eps * wo[0]
        inv = np.zeros(9, F)
        host_lib.mi_inv3(fp(A), fp(inv))
        assert np.array_equal(inv.reshape(3, 3), O.inv3(A))
        assert F(host_lib.mi_det3(fp(A))) == O.det3f(A)


def test_normalise(host_lib):
    for name in ("general_1000", "n9_it3"):
        kp = MC.scene(name)["kp1"]
        ms, T = np.zeros(4, F), np.zeros(9, F)
        host_lib.mi_normalise(fp(kp), len(kp), fp(ms), fp(T))
        mx, my, sx, sy, To = O.normalise(kp)
        assert np.array_equal(ms, np.array([mx, my, sx, sy], F)) and np.array_equal(T.reshape(3, 3), To)


@pytest.mark.parametrize("n", [8, 9, 50, 1000])
def test_samples_are_the_reference_draws(n):
    for iters in (1, 200):
        got = MI.mapinit_samples(n, iters)
        assert np.array_equal(got, O.draw_samples(n, iters))
        assert all(len(set(row)) == 8 for row in got.tolist()) and got.min() >= 0 and got.max() < n


@pytest.mark.parametrize("name", list(MC.SCENES))
def test_scene_conditions_hold_in_the_oracle(name):
    """Conditions, not measurements: at most 10 % exempt hypotheses, at most 1 % band pairs, no winner among them, and the outcome the
    scene was built for."""
    r, expect = MC.oracle(name), MC.SCENES[name][1]
    ex, band, tainted = MC.exempt_and_bands(r)
    print(f"{name}: exempt {ex.mean() if ex.size else 0:.4f}, band pairs {band:.6f}, model {r['model']}, ok {r['ok']}, n_good {r['n_good'].tolist()}")
    assert (ex.mean() if ex.size else 0.0) <= MC.MAX_EXEMPT and band <= MC.MAX_BAND and not tainted
    sc = MC.scene(name)
    if sc["plane"] is not None:   # a plane: every planted point on n . P = d
        nrm, d = sc["plane"]
        assert np.abs(sc["P"] @ nrm - d).max() <= 1e-12 * d
    if r.get("checks") and r["winner"] >= 0:   # accepted or refused: the winner's states are compared with the oracle's either way
        ch = r["checks"][r["winner"]]
        low = ch["state"] == O.COUNTED_LOW
        if name in MC.LOW_PARALLAX:
            assert low.any() and np.array_equal(ch["band"], low)   # no band case besides the low-parallax matches themselves
        else:
            assert not ch["band"].any(), "a band case in the winning candidate"
        if (expect or {}).get("behind"):
            # six planted points BEHIND both cameras at almost no parallax: the reference lets them through (counted, the point stored, the
            # keypoint not marked)
            assert low.sum() == 6 and (ch["pts"][low][:, 2] < 0).all()
            assert r["n_good"][r["winner"]] == 129 and len(r["matches"]) == 123
    for k, v in (expect or {}).items():
        if k == "n_good":
            assert r["n_good"].max() == v
        elif k == "behind":
            pass
        elif k == "rule07":
            g, N = r["n_good"][:4], r["n_inliers"]
            assert (g > 0.7 * g.max()).sum() > 1 and g.max() >= max(int(0.9 * N), 50) and r["parallax"][r["winner"]] > 1.0   # only the 0.7 rule refuses
        elif k == "rule075":
            g = np.sort(r["n_good"])
            assert g[-2] >= 0.75 * g[-1] and g[-1] > 0.9 * r["n_inliers"] and r["parallax"][r["winner"]] >= 1.0   # only the 0.75 rule refuses
        else:
            assert r[k] == v, (k, r[k], v)
    if name == "pure_rotation_129":
        assert r["parallax"][r["winner"]] < 1.0   # it fails on parallax
    if name == "duplicates_129":
        assert len(np.unique(MC.scene(name)["matches"][:, 0])) < 129


@pytest.mark.parametrize("name", list(MC.SCENES))
def test_run_host_against_the_oracle(name):
    sc, r = MC.scene(name), MC.oracle(name)
    h = MI.initialize_host(sc["intr"], sc["kp1"], sc["kp2"], sc["matches"], **sc["kw"])
    assert_agrees_with_oracle(h, r, name)
    assert np.array_equal(sc["matches"][h["index"]], h["matches"]) and (np.diff(h["index"]) > 0).all()
    if r["ok"]:   # every scene the reference accepts
        bar, err = MC.pose_bar(sc), MC.pose_error(h["R"], h["t"], sc)
        print(f"{name}: pose error {err[0]:.5f} rad / {err[1]:.5f} rad against bars {bar[0]:.5f} / {bar[1]:.5f}")
        assert err[0] <= bar[0] and err[1] <= bar[1]


def test_planted_non_finite_triangulation_host():
    sc, model, M, mask, r = MC.planted_non_finite()
    h = MI.debug_reconstruct_host(sc["intr"], sc["kp1"], sc["kp2"], sc["matches"], model, M, mask)
    assert_planted_non_finite(h, sc, r)


def test_refusals_and_the_short_input():
    sc = MC.scene("n65")
    args = (sc["intr"], sc["kp1"], sc["kp2"], sc["matches"])
    with pytest.raises(MI._lib.UcoslamHipError):
        MI.initialize_host(*args, min_matches=7)
    with pytest.raises(MI._lib.UcoslamHipError):
        MI.initialize_host(*args, iterations=0)
    bad = sc["matches"].copy()
    bad[3, 0] = len(sc["kp1"])
    with pytest.raises(MI._lib.UcoslamHipError):
        MI.initialize_host(sc["intr"], sc["kp1"], sc["kp2"], bad, min_matches=8)
    smp = O.draw_samples(65, 200)
    smp[7, 2] = 65
    with pytest.raises(MI._lib.UcoslamHipError):
        MI.initialize_host(*args, min_matches=8, samples=smp)
    h = MI.initialize_host(*args)   # 65 matches against min_matches = 50 run; 49 do not
    assert h["model"] != O.NONE
    s49 = MC.scene("n49_defaults")
    h = MI.initialize_host(s49["intr"], s49["kp1"], s49["kp2"], s49["matches"])
    assert h["ok"] == 0 and h["model"] == O.NONE and h["best_h"] == -1 and len(h["matches"]) == 0


# ---------------------------------------------------------------- the 60-digit contract (tests/golden/make_mapinit_golden.py)
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "mapinit_golden.npz"))


def test_golden_null_vectors(host_lib, golden):
    """Bar as in test_null_vectors_match_lapack: 1e-14 * sigma_1 / (sigma_8 - sigma_9), the gap taken from the golden file."""
    for key, M in (("null_h", 16), ("null_f", 8)):
        for A, ref, gap, kind in zip(golden[key + "_A"], golden[key + "_x"], golden[key + "_gap"], golden[key + "_kind"]):
            x = np.zeros(9)
            host_lib.mi_null_vector(fp(np.ascontiguousarray(A, F)), M, dp(x))
            err = np.abs(x - ref).max()
            print(f"{key} {kind}: relative gap {gap:.3e}, error {err:.3e}")
            assert err <= 1e-14 / gap, (key, kind, err, gap)


def test_golden_rank2(host_lib, golden):
    """U, w and Vt are rounded to float32 and multiplied through two float32 products: a few float roundings of the largest entry"""
    for A, ref in zip(golden["rank2_in"], golden["rank2_out"]):
        Fn = np.zeros(9, F)
        host_lib.mi_rank2(fp(np.ascontiguousarray(A, F)), fp(Fn))
        assert np.abs(Fn.reshape(3, 3) - ref).max() <= 8 * np.finfo(F).eps * np.abs(ref).max()
        assert abs(np.linalg.det(Fn.reshape(3, 3).astype(np.float64))) <= 1e-6 * np.abs(ref).max() ** 3


def _decompose(host_lib, model, Mx):
    R, t = np.zeros((8, 9), F), np.zeros((8, 3), F)
    intr = np.array([500, 500, 320, 240], F)
    n = host_lib.mi_decompose(model, fp(np.ascontiguousarray(Mx, F)), fp(intr), fp(R), fp(t))
    return n, R[:n].reshape(n, 3, 3), t[:n]


def _same_set(R, t, Rg, tg, tol):
    """every golden candidate has a partner among the computed ones and the other way round"""
    d = np.array([[max(np.abs(R[i] - Rg[j]).max(), np.abs(t[i] - tg[j]).max()) for j in range(len(Rg))] for i in range(len(R))])
    return d.min(0).max() <= tol and d.min(1).max() <= tol


def test_golden_decompositions(host_lib, golden):
    """The candidates as SETS (the sign rule fixes an order the golden file does not know).  Bar 2e-4: the float32 chain K^T F K / K^-1 H K
    carries entries up to 500^2 times the smallest through two float32 products, and U, w, Vt are rounded to float32 (6e-8 each) before
    the candidates are formed: 6e-8 * 500 * a handful of operations."""
    for F21, R1, R2, t in zip(golden["dec_f_in"], golden["dec_f_R1"], golden["dec_f_R2"], golden["dec_f_t"]):
        n, R, tt = _decompose(host_lib, O.FUNDAMENTAL, F21)
        assert n == 4 and _same_set(R, tt, [R1, R2, R1, R2], [t, t, -t, -t], 2e-4)
        assert np.array_equal(tt[0], tt[1]) and np.array_equal(tt[2], -tt[0]) and np.array_equal(R[0], R[2]) and np.array_equal(R[1], R[3])
    assert golden["dec_h_exit"].any() and not golden["dec_h_exit"].all()
    for H, d, ex, Rg, tg in zip(golden["dec_h_in"], golden["dec_h_d"], golden["dec_h_exit"], golden["dec_h_R"], golden["dec_h_t"]):
        n, R, tt = _decompose(host_lib, O.HOMOGRAPHY, H)
        print(f"singular values {d}, ratios {d[0] / d[1]:.7f} {d[1] / d[2]:.7f}, exit {bool(ex)}, candidates {n}")
        assert n == (0 if ex else 8)
        if not ex:
            # close singular values: a relative perturbation e of A turns the vectors of the close pair by e / (ratio - 1); A is formed by two
            # float32 products and U, Vt are rounded to float32: four roundings of eps = 1.2e-7, with a margin of two
            ratio = min(d[0] / d[1], d[1] / d[2])
            assert _same_set(R, tt, Rg, tg, max(2e-4, 8 * np.finfo(F).eps / (ratio - 1)))


def test_golden_triangulation(host_lib, golden):
    """The point of one match: float32 null vector of a 4x4 whose two ray pairs meet at 10 to 17 degrees; bar 1e-4 relative (float32
    rounding of the vector, 6e-8, over the sine of the parallax, times the depth-to-baseline ratio of about 5, with a margin of ten)"""
    intr = np.array([500, 500, 320, 240], F)
    for R, t, xy, X in zip(golden["tri_R"], golden["tri_t"], golden["tri_xy"], golden["tri_X"]):
        cosp, p = C.c_float(0), np.zeros(3, F)
        st = host_lib.mi_check_rt(fp(intr), fp(np.ascontiguousarray(R, F)), fp(np.ascontiguousarray(t, F)), C.c_float(4.0), fp(np.ascontiguousarray(xy, F)),
                                  C.byref(cosp), fp(p))
        assert st in (O.COUNTED_GOOD, O.REJECTED) and np.abs(p - X).max() <= 1e-4 * np.abs(X).max(), (st, p, X)


def _check_rt(host_lib, R, t, xy):
    intr = np.array([500, 500, 320, 240], F)
    cosp, p = C.c_float(0), np.zeros(3, F)
    st = host_lib.mi_check_rt(fp(intr), fp(np.ascontiguousarray(R, F)), fp(np.ascontiguousarray(t, F)), C.c_float(4.0), fp(np.ascontiguousarray(xy, F)), C.byref(cosp), fp(p))
    xy = np.asarray(xy, F)
    o = O.check_rt(np.asarray(R, F), np.asarray(t, F), intr, xy[0:1], xy[1:2], xy[2:3], xy[3:4], np.array([True]), F(4.0))
    return st, F(cosp.value), p, o


def test_check_rt_planted_states(host_lib):
    """One match each, header against oracle: a point BEHIND both cameras at low parallax, which the reference lets through (the depth
    tests are excused, the point is stored, the keypoint is not marked); the same point at a parallax that excuses nothing; a non-finite
    triangulation; a gross reprojection error."""
    R, t = np.eye(3, dtype=F), np.array([1, 0, 0], F)
    behind_far = [320, 240, 320 + 500 * 1.0 / -1000.0, 240]          # X = (0, 0, -1000): cos = 1 - 5e-7 >= 0.99998
    behind_near = [320, 240, 320 + 500 * 1.0 / -5.0, 240]            # X = (0, 0, -5): 11 degrees
    in_front = [320, 240, 320 + 500 * 1.0 / 5.0, 240]
    off_epipolar = [320, 240, 320 + 100.0, 240 + 30.0]
    not_finite = [np.inf, 240, 420, 240]
    for xy, want in ((behind_far, O.COUNTED_LOW), (behind_near, O.REJECTED), (in_front, O.COUNTED_GOOD), (off_epipolar, O.REJECTED), (not_finite, O.NON_FINITE)):
        st, cosp, p, o = _check_rt(host_lib, R, t, xy)
        assert st == want == o["state"][0], (xy, st, want, o["state"][0])
        if want != O.NON_FINITE:
            assert cosp == o["cos"][0] or abs(cosp - o["cos"][0]) <= 2 * np.finfo(F).eps
            assert np.allclose(p, o["pts"][0], rtol=1e-4)
    st, cosp, p, _ = _check_rt(host_lib, R, t, behind_far)
    assert p[2] < 0 and cosp >= F(0.99998)


def test_decision_rules_on_planted_counts(host_lib):
    """The 0.7 rule (F), the 0.75 rule (H), 0.9 N, min_triangulated and the parallax bar on planted counts: header against oracle and
    against the expected outcome, on both sides of each threshold."""
    IP = C.POINTER(C.c_int)
    cases = [   # model, N, counts, parallax of the best, expected ok
        (O.FUNDAMENTAL, 100, [100, 71, 0, 0], 2.0, 0), (O.FUNDAMENTAL, 100, [100, 70, 0, 0], 2.0, 1), (O.FUNDAMENTAL, 100, [0, 70, 100, 0], 2.0, 1),
        (O.FUNDAMENTAL, 100, [89, 0, 0, 0], 2.0, 0), (O.FUNDAMENTAL, 100, [90, 0, 0, 0], 2.0, 1), (O.FUNDAMENTAL, 40, [40, 0, 0, 0], 2.0, 0),
        (O.FUNDAMENTAL, 100, [100, 0, 0, 0], 1.0, 0), (O.FUNDAMENTAL, 100, [100, 100, 0, 0], 2.0, 0),
        (O.HOMOGRAPHY, 100, [100, 75, 0, 0, 0, 0, 0, 0], 2.0, 0), (O.HOMOGRAPHY, 100, [100, 74, 0, 0, 0, 0, 0, 0], 2.0, 1),
        (O.HOMOGRAPHY, 100, [10, 74, 0, 0, 0, 100, 0, 0], 2.0, 1), (O.HOMOGRAPHY, 100, [90, 0, 0, 0, 0, 0, 0, 0], 2.0, 0),
        (O.HOMOGRAPHY, 100, [91, 0, 0, 0, 0, 0, 0, 0], 1.0, 1), (O.HOMOGRAPHY, 100, [91, 0, 0, 0, 0, 0, 0, 0], 0.99, 0),
        (O.HOMOGRAPHY, 55, [50, 0, 0, 0, 0, 0, 0, 0], 2.0, 0), (O.HOMOGRAPHY, 55, [51, 0, 0, 0, 0, 0, 0, 0], 2.0, 1),
        (O.HOMOGRAPHY, 100, [100, 100, 0, 0, 0, 0, 0, 0], 2.0, 0),
    ]
    for model, N, counts, par, want in cases:
        g = np.zeros(8, np.int32)
        g[:len(counts)] = counts
        pr = np.zeros(8, F)
        pr[int(np.argmax(g))] = par
        w = C.c_int(-2)
        ok = host_lib.mi_decide(model, len(counts), N, g.ctypes.data_as(IP), fp(pr), C.c_float(1.0), 50, C.byref(w))
        ok_o, w_o = O.decide(model, [None] * len(counts), N, g, pr, 1.0, 50)
        assert ok == want == int(ok_o) and w.value == w_o == int(np.argmax(g)), (model, N, counts, par, ok, ok_o, w.value, w_o)
