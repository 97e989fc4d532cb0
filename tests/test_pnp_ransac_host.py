"""Relocalisation RANSAC, the part that needs no GPU: the scenes and constructed cases of tests/test_pnp_ransac.py are fixed against the
numpy oracle ALONE (every solution checked on its own, share of near-threshold pairs, share of ill-conditioned hypotheses), a host
build of the kernel's arithmetic (csrc/p3p_math.hpp) is compared with the oracle on every fixture hypothesis, the sampler is compared
with the real std::random_shuffle, and the validation paths of uh_pnp_ransac that return before any launch are visited."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pnp_ransac_cases as PC
import pnp_ransac_oracle as O
import pnp_ransac_synth as S
from pnp_ransac_cases import POSE_BARS, TOL, planted_pose_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = list(S.PARITY) + list(S.PLANTED)


def P(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- the oracle alone

@pytest.mark.parametrize("name", SCENES)
def test_scene_is_fixed_by_the_oracle_alone(name):
    pr, r = PC.scene_and_oracle(name)
    pairs = pr["n"] * pr["iters"]
    near = sum(PC.band_pairs(h) for h in r["hyp"])
    ill = sum(bool(h["ill"]) for h in r["hyp"])
    worst = max([O.check_solution(pr["intr"], h["P"], h["px"], s) for h in r["hyp"] for s in h["solutions"]], default=0.0)
    print(f"{name}: {pr['iters']} hypotheses x {pr['n']} matches, {near} pairs in the band, {ill} ill-conditioned, solutions "
          f"{np.bincount([h['n_solutions'] for h in r['hyp']], minlength=5).tolist()}, worst self-check {worst:.3g}")
    assert near <= O.MAX_NEAR_SHARE * pairs               # (i)
    assert ill <= O.MAX_ILL_SHARE * pr["iters"]            # (ii)
    # every solution on its own: R'R = I, det R = +1, the three sample points on their pixels (normalised), distances positive
    assert worst <= 1e-9


@pytest.mark.parametrize("name", list(S.PLANTED))
def test_planted_scene_recovers_its_inliers(name):
    pr, r = PC.scene_and_oracle(name)
    h = r["hyp"][r["best_iter"]]
    keep = h["margin"] >= O.NEAR
    # the inlier list equals the planted inliers outside the band (noise 0.3 px against a gate of 2.45 px: 8 sigma)
    assert r["ok"] == 1 and np.array_equal(h["mask"][keep], pr["planted_inlier"][keep])
    # "within the noise": a pose that brings every planted inlier, spread over the whole image, within the gate of sqrt(5.99) = 2.45 px
    # of its keypoint is rotated by at most about 2.45 / fx = 3.4e-3 rad against the planted one and shifted by at most about that
    # angle times the largest depth (10): bars of three times those figures
    dR, dt = planted_pose_error(pr, r["rt6"])
    assert dR <= POSE_BARS[0] and dt <= POSE_BARS[1]


def test_constructed_cases_against_their_expectations():
    pr, r = PC.repeated_sample()
    assert r["best_iter"] == 2 and r["counts"][2] == r["counts"][7] == r["counts"].max() and (np.delete(r["counts"], [2, 7]) < r["counts"][2]).all()
    pr, r = PC.collinear()
    assert (r["counts"] == -1).all() and r["ok"] == 0 and r["best_iter"] == -1 and np.array_equal(r["rt6"], pr["rt6_in"])
    pr, r = PC.best_of_three()
    assert r["counts"].tolist() == [3] and r["ok"] == 0 and r["best_iter"] == 0 and not np.array_equal(r["rt6"], pr["rt6_in"])
    assert r["inliers"].tolist() == [0, 1, 2] and (r["hyp"][0]["margin"] >= O.NEAR).all()
    pr, r = PC.special_points()
    h = r["hyp"][0]
    assert h["mask"].tolist() == PC.SPECIAL_EXPECT and (h["margin"] >= O.NEAR).all()
    M = O.se3_set(h["rt6"])
    z = M[8] * pr["p3d"][:, 0] + M[9] * pr["p3d"][:, 1] + M[10] * pr["p3d"][:, 2] + M[11]
    assert z[4] < -1 and abs(z[5]) < 1e-5 and h["err2"][4] < 1e-3            # behind the camera, inside the gate: an inlier
    assert h["err2"][6] < 1e-3 and 0.48 < h["viewcos"][6] < 0.4999          # reprojects exactly, seen too obliquely


def test_rodrigues_branches_against_the_oracle(math_host):
    """matrix -> vector near theta = 0, in the general range and near theta = pi, against the oracle's eigenvector route."""
    rng = np.random.default_rng(3)
    worst = 0.0
    for theta in (0.0, 1e-9, 1e-6, 3e-5, 0.3, 2.0, 3.1, np.pi - 3e-6, np.pi - 1e-9, np.pi):
        for _ in range(6):
            ax = rng.normal(size=3)
            ax /= np.linalg.norm(ax)
            R = np.ascontiguousarray(S.rodrigues(ax * theta))
            got = np.zeros(3)
            math_host.p3p_host_rodrigues(P(R), P(got))
            worst = max(worst, np.abs(S.rodrigues(got) - R).max())
            assert abs(np.linalg.norm(got) - theta) < 1e-7
    print(f"rodrigues round trip: worst |R(r) - R| {worst:.3g}")
    assert worst < 1e-9


# ---- the kernel's arithmetic on the host

@pytest.fixture(scope="module")
def math_host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("p3p") / "libp3p_math_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                           os.path.join(ROOT, "tests", "host_helpers", "p3p_math_host.cpp")])
    return C.CDLL(so)


def host_hypothesis(L, pr, it):
    idx = pr["samples"][it]
    Pf, pf = np.ascontiguousarray(pr["p3d"][idx]), np.ascontiguousarray(pr["kp"][idx])
    Rt, ch, rt6, rv = np.zeros((4, 12)), C.c_int(0), np.zeros(6, np.float32), np.zeros(6)
    ns = L.p3p_host_hypothesis(P(pr["intr"]), P(Pf), P(pf), P(Rt), C.byref(ch), P(rt6), P(rv))
    return dict(n_solutions=ns, Rt=Rt[:ns], chosen=ch.value, rt6=rt6, rvec_tvec=rv)


def compare_hypothesis(got, h):
    """(worst distance of a solution, rt6 bits equal) of a well-conditioned hypothesis; asserts the discrete parts."""
    assert got["n_solutions"] == h["n_solutions"] and got["chosen"] == h["chosen"]
    worst = 0.0
    for k, s in enumerate(h["solutions"]):
        worst = max(worst, np.abs(got["Rt"][k, :9].reshape(3, 3) - s["R"]).max(), np.abs(got["Rt"][k, 9:] - s["t"]).max())
    return worst


@pytest.mark.parametrize("name", SCENES + ["repeated", "collinear", "three", "special"])
def test_host_build_of_the_kernel_arithmetic_against_the_oracle(math_host, name):
    """Number of solutions, every solution, chosen index, rt6 bits and inlier masks of every fixture hypothesis.  rt6: the float cast
    of two doubles that differ by ~1e-12 can fall on either side of a float rounding boundary (probability ~1e-5 per value), so the
    bits are compared wherever the doubles agree to 1e-3 of a float ulp, and the masks are taken with the oracle's rt6.
    Observed: worst solution distance 2.3e-12 (2.9e-9 before the oracle refined its distances), rt6 bits equal everywhere."""
    cases = {"repeated": PC.repeated_sample, "collinear": PC.collinear, "three": PC.best_of_three, "special": PC.special_points}
    pr, r = cases[name]() if name in cases else PC.scene_and_oracle(name)
    worst = 0.0
    for it, h in enumerate(r["hyp"]):
        if h["ill"]:
            continue
        got = host_hypothesis(math_host, pr, it)
        worst = max(worst, compare_hypothesis(got, h))
        if h["chosen"] < 0:
            continue
        ulp = np.spacing(np.abs(h["rt6"]).astype(np.float32)).astype(np.float64)
        sure = np.abs(got["rvec_tvec"] - h["rvec_tvec"]) < 1e-3 * ulp
        near_tie = np.abs(np.abs(h["rvec_tvec"] - h["rt6"].astype(np.float64)) - 0.5 * ulp) < 1e-3 * ulp
        assert np.array_equal(got["rt6"][sure & ~near_tie], h["rt6"][sure & ~near_tie])
        mask = np.zeros(pr["n"], np.uint8)
        cnt = math_host.p3p_host_score(P(pr["intr"]), P(h["rt6"]), pr["n"], P(pr["p3d"]), P(pr["normal"]), P(pr["kp"]), P(mask), None, None)
        keep = h["margin"] >= O.NEAR
        assert np.array_equal(mask.astype(bool)[keep], h["mask"][keep])
        assert abs(cnt - h["count"]) <= PC.band_pairs(h)
    print(f"{name}: host build against the oracle, worst solution distance {worst:.3g}")
    assert worst <= TOL


def test_host_loop_picks_the_oracles_winner(math_host):
    for name in S.PLANTED:
        pr, r = PC.scene_and_oracle(name)
        counts, rt6 = np.zeros(pr["iters"], np.int32), np.zeros(6, np.float32)
        best = math_host.p3p_host_ransac(P(pr["intr"]), pr["n"], P(pr["p3d"]), P(pr["normal"]), P(pr["kp"]), pr["iters"], P(pr["samples"]), P(counts), P(rt6))
        band = np.array([PC.band_pairs(h) for h in r["hyp"]])
        assert (np.abs(counts - r["counts"]) <= band).all()
        if band.sum() == 0:
            assert best == r["best_iter"] and np.array_equal(rt6, r["rt6"])


# ---- the sampler

@pytest.fixture(scope="module")
def shuffle_ref(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("shuf") / "librandom_shuffle_ref.so")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wno-deprecated-declarations", "-shared", "-fPIC", "-o", so,
                           os.path.join(ROOT, "tests", "host_helpers", "random_shuffle_ref.cpp")])
    return C.CDLL(so)


@pytest.mark.parametrize("n", [4, 5, 64, 500])
@pytest.mark.parametrize("seed", [0, 1, 20240607])
def test_sampler_draws_what_std_random_shuffle_draws(shuffle_ref, n, seed):
    from ucoslam_cv3_amd import ransac_samples

    libc = C.CDLL(None)
    want, nxt = np.zeros((50, 4), np.int32), C.c_int(0)
    shuffle_ref.ref_shuffle_samples(C.c_uint(seed), n, 50, P(want), C.byref(nxt))
    libc.srand(C.c_uint(seed))
    got = ransac_samples(n, 50)
    assert np.array_equal(got, want)
    assert libc.rand() == nxt.value            # rand() is left where the reference leaves it
    assert all(len(set(row)) == 4 for row in got.tolist())


# ---- uh_pnp_ransac: what returns before any launch (no GPU, no solver object)

def _call(intr, problems, caps=None, n_problems=None, null_results=False):
    from ucoslam_cv3_amd import lib, pnp_ransac as PR

    keep = []
    m = len(problems)
    ps, rs = (PR._Problem * max(m, 1))(), (PR._Result * max(m, 1))()
    bufs = []
    for j, pr in enumerate(problems):
        ps[j] = PR._pack(pr, keep)
        inl, cnt = np.full(max(ps[j].n, 1), -7, np.int32), np.full(max(ps[j].iters, 1), -7, np.int32)
        bufs.append((inl, cnt))
        rs[j].inliers, rs[j].cap, rs[j].counts = P(inl), (ps[j].n if caps is None else caps[j]), P(cnt)
    intr = np.ascontiguousarray(intr, np.float32)
    rc = lib().uh_pnp_ransac(None, P(intr), m if n_problems is None else n_problems, C.cast(ps, C.c_void_p), None if null_results else C.cast(rs, C.c_void_p))
    return rc, lib().uh_last_error().decode(), rs, bufs


def _small(n=8, iters=3):
    pr = dict(S.scene(7, max(n, 4), iters, outliers=0.0))
    out = {k: pr[k] for k in ("p3d", "normal", "kp", "samples", "rt6_in")}
    if n < 4:   # below four matches no sample exists
        out.update(p3d=pr["p3d"][:n], normal=pr["normal"][:n], kp=pr["kp"][:n], samples=np.zeros((iters, 4), np.int32), n=n)
    return out


def test_refusals_before_any_launch():
    EINVAL = -1
    ok = _small()
    cases = []
    bad = dict(ok); bad["samples"] = ok["samples"].copy(); bad["samples"][1, 2] = 8
    cases.append(("outside", [bad], {}))
    bad = dict(ok); bad["samples"] = ok["samples"].copy(); bad["samples"][2, 0] = -1
    cases.append(("outside", [bad], {}))
    bad = dict(ok); bad["samples"] = ok["samples"].copy(); bad["samples"][0, 3] = bad["samples"][0, 1]
    cases.append(("twice", [bad], {}))
    cases.append(("inlier buffer", [ok], dict(caps=[7])))
    cases.append(("iterations outside", [dict(ok, iters=1025, samples=np.zeros((1025, 4), np.int32))], {}))
    cases.append(("iterations outside", [dict(ok, iters=0)], {}))
    cases.append(("matches outside", [dict(ok, n=16385)], {}))
    cases.append(("problems outside", [ok], dict(n_problems=65)))
    cases.append(("NULL problem or result", [ok], dict(null_results=True)))
    for text, problems, kw in cases:
        rc, msg, _, _ = _call(S.INTR, problems, **kw)
        assert rc == EINVAL and text in msg, (text, rc, msg)
    for k in range(4):
        intr = S.INTR.copy()
        intr[k] = [np.nan, np.inf, -np.inf, np.nan][k]
        rc, msg, _, _ = _call(intr, [ok])
        assert rc == EINVAL and "non-finite intrinsics" in msg
    # NULL arrays with n > 0
    from ucoslam_cv3_amd import lib, pnp_ransac as PR
    keep = []
    q = PR._pack(ok, keep)
    q.normal = None
    r = PR._Result()
    inl = np.zeros(8, np.int32)
    r.inliers, r.cap = P(inl), 8
    assert lib().uh_pnp_ransac(None, P(S.INTR), 1, C.byref(q), C.byref(r)) == EINVAL and "NULL match arrays" in lib().uh_last_error().decode()
    # a well-formed call with something to launch and no solver is refused as well, after every check above
    rc, msg, _, _ = _call(S.INTR, [ok])
    assert rc == EINVAL and "NULL solver" in msg


def test_nothing_to_launch_returns_without_a_device():
    rc, _, _, _ = _call(S.INTR, [], n_problems=0)
    assert rc == 0
    small = _small(3, 5)
    rc, msg, rs, bufs = _call(S.INTR, [small, _small(0, 2)])
    assert rc == 0, msg
    for j, iters in ((0, 5), (1, 2)):
        r = rs[j]
        assert (r.ok, r.n_inliers, r.best_iter) == (0, 0, -1)
        assert np.array_equal(np.array(r.rt6[:], np.float32), small["rt6_in"])
        assert np.array_equal(np.array(r.pose[:], np.float32)[:12], O.se3_set(small["rt6_in"]))
        assert (bufs[j][1][:iters] == -1).all() and (bufs[j][0] == -7).all()      # matches_io is untouched
