"""New map points, the part that needs no GPU: the scenes and constructed cases of tests/test_newpoints.py are fixed against the numpy
oracle ALONE (share of near-threshold matches, branch codes, merge expectations), the 1-ulp bar is shown to be the oracle's own
reproducibility (np.linalg.svd of A against np.linalg.eigh of A'A), the kernel's Jacobi sweep count is re-derived from a host build
of the kernel's arithmetic (csrc/newpoints_math.hpp), and uh_fundamental_12 (host code of the library) is checked."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import newpoints_cases as NC
import newpoints_oracle as O
import newpoints_synth as S
from newpoints_oracle import MAX_NEAR_SHARE, NEAR, ulp_diff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

@pytest.fixture(scope="module")
def scenes():
    out = {}
    for name in S.CASES:
        kf, pairs = S.case(name)
        out[name] = (kf, pairs, O.run(kf, pairs, ratio_factor=S.RATIO_FACTOR))
    return out


@pytest.mark.parametrize("name", list(S.CASES))
def test_scene_is_fixed_by_the_oracle_alone(scenes, name):
    kf, pairs, r = scenes[name]
    n = len(r["status"])
    near = int((r["margin"] < NEAR).sum())
    print(f"{name}: {n} matches, status histogram {np.bincount(r['status'], minlength=10).tolist()}, {near} near a threshold, n_new {r['n_new']}")
    assert near <= MAX_NEAR_SHARE * n
    for p in pairs:   # the property the kernels rely on
        assert len(np.unique(p["matches"]["trainIdx"])) == len(p["matches"])


def test_wide_scene_visits_the_common_branches(scenes):
    hist = np.bincount(scenes["wide"][2]["status"], minlength=10)
    assert hist[0] > 4000 and all(hist[c] > 0 for c in (1, 4, 6, 7, 9))


@pytest.mark.parametrize("name", list(S.CASES))
def test_one_ulp_is_the_oracles_own_reproducibility(scenes, name):
    """Second CPU path: eigh of A'A in float64 instead of svd of A.  Flags equal, coordinates within 1 ulp (observed: 0 on every scene)."""
    kf, pairs, r = scenes[name]
    r2 = O.run(kf, pairs, ratio_factor=S.RATIO_FACTOR, null="eigh")
    keep = r["margin"] >= NEAR
    assert np.array_equal(r["status"][keep], r2["status"][keep])
    both = keep & np.isfinite(r["xyz_cam"]).all(1)
    worst = int(ulp_diff(r["xyz_cam"][both], r2["xyz_cam"][both]).max(initial=0))
    print(f"{name}: svd against eigh, worst {worst} ulp over {int(both.sum())} points")
    assert worst <= 1


@pytest.mark.parametrize("name", list(NC.BRANCH))
def test_branch_case_reaches_its_branch(name):
    build, code = NC.BRANCH[name]
    kf, pairs = build()
    r = O.run(kf, pairs, ratio_factor=S.RATIO_FACTOR)
    assert r["status"].tolist() == [code], O.__name__
    assert (r["margin"] >= NEAR).all()
    assert r["n_new"] == (1 if code == 0 else 0)


def test_merge_scene_against_its_hand_derived_expectations():
    kf, pairs, ex = NC.merge_scene()
    r = O.run(kf, pairs, ratio_factor=S.RATIO_FACTOR)
    assert (r["margin"] >= NEAR).all()
    assert r["status"].tolist() == [0, 0, 6, 0, 0, 0, 0, 0]
    assert r["kp_idx"].tolist() == ex["kp_idx"] and r["chosen_pair"].tolist() == ex["chosen_pair"]
    assert r["obs_ptr"].tolist() == ex["obs_ptr"] and r["obs_pair"].tolist() == ex["obs_pair"]
    # the observed keypoints: the new keyframe's own index first, then the neighbours' (stored reversed: 3 - q, the last pair has 4)
    assert r["obs_kpt"].tolist() == [0, 3, 3, 3, 1, 2, 2, 2, 3, 0]
    last = O.run(kf, pairs, ratio_factor=S.RATIO_FACTOR, merge_rule=O.MERGE_LAST)
    assert last["chosen_pair"].tolist() == ex["chosen_pair_as_compiled"] and last["obs_pair"].tolist() == ex["obs_pair"]


# ---- the kernel's arithmetic on the host

@pytest.fixture(scope="module")
def math_host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("npm") / "libnewpoints_math_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                           os.path.join(ROOT, "tests", "host_helpers", "newpoints_math_host.cpp")])
    return C.CDLL(so)


def _host_pair(L, kf, pair, sweeps):
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    m = pair["matches"]
    n = len(m)
    pt1, o1 = np.ascontiguousarray(kf["pt"][m["trainIdx"]]), np.ascontiguousarray(kf["octave"][m["trainIdx"]])
    pt2, o2 = np.ascontiguousarray(pair["pt"][m["queryIdx"]]), np.ascontiguousarray(pair["octave"][m["queryIdx"]])
    cam, glob, st = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.uint8)
    T = np.ascontiguousarray(kf["pose_g2f"][:3, :].reshape(12))
    L.np_host_triangulate(P(kf["intr4"]), P(T), P(kf["cam_center"]), C.c_float(5.998), C.c_float(S.RATIO_FACTOR), P(kf["scale_factors"]),
                          P(np.ascontiguousarray(pair["RT"])), P(pair["intr4"]), P(pair["cam_center"]), P(pair["scale_factors"]), n, P(pt1), P(o1),
                          P(pt2), P(o2), sweeps, P(cam), P(glob), P(st))
    return cam, glob, st


def _agrees(L, kf, pairs, r, sweeps):
    for j, p in enumerate(pairs):
        cam, glob, st = _host_pair(L, kf, p, sweeps)
        sl = slice(r["pair_offset"][j], r["pair_offset"][j + 1])
        keep = r["margin"][sl] >= NEAR
        if not np.array_equal(st[keep], r["status"][sl][keep]):
            return False
        if not np.array_equal(np.isnan(cam[keep]), np.isnan(r["xyz_cam"][sl][keep])):
            return False
        fin = keep & np.isfinite(r["xyz_cam"][sl]).all(1)
        acc = keep & (r["status"][sl] == 0)
        if ulp_diff(cam[fin], r["xyz_cam"][sl][fin]).max(initial=0) > 1 or ulp_diff(glob[acc], r["match_xyz_global"][sl][acc]).max(initial=0) > 1:
            return False
    return True


def test_jacobi_sweep_count_is_the_smallest_that_agrees_plus_one(scenes, math_host):
    """The kernel's fixed sweep count: the smallest count at which EVERY fixture match (scenes, branch cases, merge scene) agrees with
    the oracle — flags equal, coordinates within 1 ulp — plus one.  Observed: 4, so kJacobiSweeps = 5."""
    fixtures = [(kf, pairs, r) for (kf, pairs, r) in scenes.values()]
    for build, _code in NC.BRANCH.values():
        kf, pairs = build()
        fixtures.append((kf, pairs, O.run(kf, pairs, ratio_factor=S.RATIO_FACTOR)))
    kf, pairs, _ex = NC.merge_scene()
    fixtures.append((kf, pairs, O.run(kf, pairs, ratio_factor=S.RATIO_FACTOR)))
    ok = {s: all(_agrees(math_host, kf, pairs, r, s) for (kf, pairs, r) in fixtures) for s in range(1, 9)}
    print("sweeps -> every fixture agrees:", ok)
    smallest = min(s for s, good in ok.items() if good)
    assert all(ok[s] for s in range(smallest, 9))
    assert math_host.np_host_default_sweeps() == smallest + 1


# ---- uh_fundamental_12

def _pairs_for_f12():
    rng = np.random.default_rng(5)
    out = []
    for k in range(20):
        p1 = S.pose(rng.normal(0, 0.2, 3), rng.normal(0, 1, 3))
        p2 = S.pose(rng.normal(0, 0.2, 3), rng.normal(0, 1, 3))
        i1 = (S.INTR * rng.uniform(0.8, 1.25, 4)).astype(np.float32)
        i2 = (S.INTR * rng.uniform(0.8, 1.25, 4)).astype(np.float32)
        out.append((p1, p2, i1, i2, O._mm(p2, S.se3_inv(p1))))
    return out


def test_fundamental_12_against_float64():
    """Bar: 1e-5 * max|F| (about a dozen float roundings through two inverses of well-conditioned K).  Observed: at most 1.01e-6 * max|F|
    against float64; the library and the oracle's float chain are equal bit for bit."""
    from ucoslam_cv3_amd.newpoints import fundamental_12

    worst = 0.0
    for (p1, p2, i1, i2, RT) in _pairs_for_f12():
        F = fundamental_12(i1, i2, RT)
        F64 = O.fundamental_12_f64(i1, i2, RT)
        rel = float(np.abs(F - F64).max() / np.abs(F64).max())
        worst = max(worst, rel)
        assert rel <= 1e-5
        assert np.array_equal(F, O.fundamental_12(i1, i2, RT))
    print(f"uh_fundamental_12 against float64: worst {worst:.3g} * max|F|")


def test_fundamental_12_puts_exact_correspondences_on_their_epipolar_lines():
    """epipolarLineSqDist(trainKp, queryKp, F12) (misc.h:72-85, as framematcher.cpp:261 calls it) of noise-free correspondences against the
    matcher's gate 3.84 * scaleFactor^2 at octave 0: below it by a wide factor, which is printed."""
    from ucoslam_cv3_amd.newpoints import fundamental_12

    rng = np.random.default_rng(6)
    worst = 0.0
    for (p1, p2, i1, i2, RT) in _pairs_for_f12()[:8]:
        F = fundamental_12(i1, i2, RT)
        c = S.cam_center(p1).astype(np.float64)
        X = c + (rng.uniform(-1, 1, (50, 3)) * [2, 2, 0] + [0, 0, 1]) @ p1[:3, :3].astype(np.float64) * rng.uniform(3, 9, (50, 1))
        x1, x2 = S.project(p1, i1, X).astype(np.float32), S.project(p2, i2, X).astype(np.float32)
        front = (X @ p2[:3, :3].astype(np.float64).T + p2[:3, 3])[:, 2] > 0.5
        for a, b in zip(x1[front], x2[front]):
            worst = max(worst, float(O.epipolar_line_sq_dist(a, b, F)))
    gate = 3.84 * float(S.SCALE_FACTORS[0]) ** 2
    print(f"worst epipolar distance^2 of exact correspondences {worst:.3g} px^2: {gate / worst:.3g} times below the gate {gate}")
    assert worst * 100 < gate
