"""Relocalisation RANSAC on the device (uh_pnp_ransac) against the numpy oracle, through the C ABI and its debug hook.  The scenes and
constructed cases are the ones tests/test_pnp_ransac_host.py fixes against the oracle alone (shares of near-threshold pairs and of
ill-conditioned hypotheses, every expectation of the constructed cases).

Sizes: n in {4, 5, 63, 64, 65, 129, 257, 1000} (the mask word and wave-stride edges), iterations in {1, 3, 4, 5, 50} (the
four-waves-per-workgroup edge), 1-3 problems of unequal n and iterations in one call."""
import numpy as np
import pytest

import pnp_ransac_cases as PC
import pnp_ransac_oracle as O
import pnp_ransac_synth as S
from pnp_ransac_cases import POSE_BARS, TOL, planted_pose_error

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ransac(hip_ctx):
    from ucoslam_cv3_amd import PnPRansac

    r = PnPRansac(hip_ctx)
    yield r
    r.close()


def check_against_oracle(pr, r, got, hook=None):
    """One problem's result against the oracle's: counts up to the band pairs of each hypothesis; with no band pair anywhere also the
    winner, its rt6 bits (hook: iteration -> the debug hook's result for this problem), pose and inlier list."""
    band = np.array([PC.band_pairs(h) for h in r["hyp"]])
    ill = np.array([bool(h["ill"]) for h in r["hyp"]])
    ok = ~ill
    skipped_o, skipped_g = r["counts"] < 0, got["counts"] < 0
    assert np.array_equal(skipped_o[ok], skipped_g[ok])
    live = ok & ~skipped_o
    assert (np.abs(got["counts"][live] - r["counts"][live]) <= band[live]).all()
    if band.sum() == 0 and not ill.any():
        assert got["best_iter"] == r["best_iter"] and got["n_inliers"] == r["n_inliers"] and got["ok"] == r["ok"]
        assert np.array_equal(got["inliers"], r["inliers"])
        if r["best_iter"] >= 0 and hook is not None:
            # the winner's rt6 as the call returns it: the float cast of the device's own doubles, and the oracle's bits (PC.rt6_must_equal)
            h = r["hyp"][r["best_iter"]]
            d = hook(r["best_iter"])
            assert got["rt6"].tobytes() == d["rvec_tvec"].astype(np.float32).tobytes()
            must = PC.rt6_must_equal(h, d["rvec_tvec"])
            assert np.array_equal(got["rt6"][must], h["rt6"][must])
        assert np.array_equal(got["pose"].reshape(16)[:12], O.se3_set(got["rt6"])) and got["pose"][3].tolist() == [0, 0, 0, 1]


@pytest.mark.parametrize("name", list(S.PARITY))
def test_scene_against_the_oracle(ransac, name):
    """Debug hook: number of solutions and chosen index equal, every solution's R, t within 1e-6 of the oracle's, rt6 equal, on the
    well-conditioned hypotheses; the whole call: counts, winner, inliers.  Observed worst solution distance: see
    profiles/pnp_ransac_parity.txt."""
    worst, compared, exempt, differ = hook_against_oracle(ransac, *PC.scene_and_oracle(name))
    print(f"{name}: device against the oracle, worst solution distance {worst:.3g}; rt6: {compared} components asserted equal bit for bit, "
          f"{exempt} exempt (a float rounding tie between the two doubles), {differ} of those differ")
    assert worst <= TOL


def hook_against_oracle(ransac, pr, r):
    """The whole call, then the debug hook on EVERY well-conditioned hypothesis of the problem: number of solutions and chosen index equal,
    every solution within TOL, the chosen (rvec, tvec) within TOL and its float cast equal to the oracle's rt6 bit for bit except where a
    rounding tie lies between the two doubles (PC.rt6_must_equal).  Returns (worst distance, components asserted, exempt, exempt and different)."""
    got = ransac.solve(pr["intr"], [pr])[0]
    check_against_oracle(pr, r, got, hook=lambda it: ransac.debug_hypothesis(pr["intr"], pr, it))
    worst, compared, exempt, differ = 0.0, 0, 0, 0
    for it, h in enumerate(r["hyp"]):
        if h["ill"]:
            continue
        d = ransac.debug_hypothesis(pr["intr"], pr, it)
        assert d["n_solutions"] == h["n_solutions"] and d["chosen"] == h["chosen"]
        for k, s in enumerate(h["solutions"]):
            worst = max(worst, np.abs(d["Rt"][k, :9].reshape(3, 3) - s["R"]).max(), np.abs(d["Rt"][k, 9:] - s["t"]).max())
        if h["chosen"] >= 0:
            assert np.abs(d["rvec_tvec"] - h["rvec_tvec"]).max() <= TOL
            dev = d["rvec_tvec"].astype(np.float32)
            must = PC.rt6_must_equal(h, d["rvec_tvec"])
            assert np.array_equal(dev[must], h["rt6"][must]), (it, dev, h["rt6"])
            compared += int(must.sum()); exempt += int((~must).sum()); differ += int((dev[~must] != h["rt6"][~must]).sum())
    return worst, compared, exempt, differ


@pytest.mark.parametrize("names", [("n65_it50", "n4_it1"), ("n5_it3", "n1000_it50", "n64_it5"), ("n129_it4", "n63_it4", "n257_it5")])
def test_unequal_problems_in_one_call(ransac, names):
    prs = [PC.scene_and_oracle(n) for n in names]
    got = ransac.solve(S.INTR, [pr for pr, _ in prs])
    for (pr, r), g in zip(prs, got):
        check_against_oracle(pr, r, g, hook=lambda it, pr=pr: ransac.debug_hypothesis(pr["intr"], pr, it))
    alone = [ransac.solve(S.INTR, [pr])[0] for pr, _ in prs]
    for g, a in zip(got, alone):   # a problem's result does not depend on its neighbours in the call
        assert g["best_iter"] == a["best_iter"] and np.array_equal(g["counts"], a["counts"]) and np.array_equal(g["inliers"], a["inliers"])
        assert g["rt6"].tobytes() == a["rt6"].tobytes()


def test_first_of_two_equal_hypotheses_wins(ransac):
    pr, r = PC.repeated_sample()
    got = ransac.solve(pr["intr"], [pr])[0]
    assert got["counts"][2] == got["counts"][7] == got["counts"].max() and got["best_iter"] == 2
    assert hook_against_oracle(ransac, pr, r)[0] <= TOL


def test_collinear_samples_are_skipped(ransac):
    pr, r = PC.collinear()
    got = ransac.solve(pr["intr"], [pr])[0]
    assert (got["counts"] == -1).all() and (got["ok"], got["n_inliers"], got["best_iter"]) == (0, 0, -1)
    assert np.array_equal(got["rt6"], pr["rt6_in"]) and np.array_equal(got["pose"].reshape(16)[:12], O.se3_set(pr["rt6_in"]))


def test_best_count_of_three_overwrites_the_pose_and_fails(ransac):
    pr, r = PC.best_of_three()
    got = ransac.solve(pr["intr"], [pr])[0]
    assert (got["ok"], got["n_inliers"], got["best_iter"]) == (0, 3, 0) and got["inliers"].tolist() == [0, 1, 2]
    assert not np.array_equal(got["rt6"], pr["rt6_in"])
    assert hook_against_oracle(ransac, pr, r)[0] <= TOL


def test_behind_the_camera_counts_camera_plane_and_oblique_view_do_not(ransac):
    pr, r = PC.special_points()
    got = ransac.solve(pr["intr"], [pr])[0]
    mask = np.zeros(pr["n"], bool)
    mask[got["inliers"]] = True
    assert mask.tolist() == PC.SPECIAL_EXPECT and got["ok"] == 1


def test_three_matches_beside_a_hundred(ransac):
    big = S.scene(77, 100, 5, outliers=0.3)
    small = dict(p3d=big["p3d"][:3], normal=big["normal"][:3], kp=big["kp"][:3], samples=np.zeros((4, 4), np.int32), rt6_in=big["rt6_in"], n=3)
    a, b = ransac.solve(S.INTR, [small, big])
    assert (a["ok"], a["n_inliers"], a["best_iter"]) == (0, 0, -1) and np.array_equal(a["rt6"], big["rt6_in"]) and (a["counts"] == -1).all()
    check_against_oracle(big, O.run(big), b, hook=lambda it: ransac.debug_hypothesis(S.INTR, big, it))
    b2, a2 = ransac.solve(S.INTR, [big, small])
    assert np.array_equal(b2["inliers"], b["inliers"]) and b2["rt6"].tobytes() == b["rt6"].tobytes() and a2["ok"] == 0


def test_both_root_forms_give_the_same_bits(ransac):
    """The measurement hook's other form of the hypothesis kernel (every lane takes all four roots) against the built one (one root per lane)."""
    prs = [PC.scene_and_oracle(n)[0] for n in ("n1000_it50", "n65_it50", "out60", "n4_it1")] + [PC.collinear()[0], PC.special_points()[0]]
    one = ransac.solve(S.INTR, prs)
    ransac.set_form(True)
    try:
        two = ransac.solve(S.INTR, prs)
    finally:
        ransac.set_form(False)
    for a, b in zip(one, two):
        assert (a["ok"], a["n_inliers"], a["best_iter"]) == (b["ok"], b["n_inliers"], b["best_iter"])
        for k in ("rt6", "pose", "inliers", "counts"):
            assert a[k].tobytes() == b[k].tobytes()


def test_two_runs_are_bit_identical(ransac):
    prs = [PC.scene_and_oracle(n)[0] for n in ("n1000_it50", "n65_it50", "out60")]
    one, two = ransac.solve(S.INTR, prs), ransac.solve(S.INTR, prs)
    for a, b in zip(one, two):
        assert (a["ok"], a["n_inliers"], a["best_iter"]) == (b["ok"], b["n_inliers"], b["best_iter"])
        for k in ("rt6", "pose", "inliers", "counts"):
            assert a[k].tobytes() == b[k].tobytes()


@pytest.mark.parametrize("name", list(S.PLANTED))
def test_planted_scene(ransac, name):
    """30 % and 60 % gross outliers, 50 iterations: the inlier list equals the planted inliers outside the band, and the pose is within
    the noise of the planted pose (the bars are derived in tests/pnp_ransac_cases.py)."""
    pr, r = PC.scene_and_oracle(name)
    worst, compared, exempt, differ = hook_against_oracle(ransac, pr, r)
    print(f"{name}: worst solution distance {worst:.3g}; rt6: {compared} asserted, {exempt} exempt, {differ} of those differ")
    assert worst <= TOL
    got = ransac.solve(pr["intr"], [pr])[0]
    assert got["ok"] == 1
    mask = np.zeros(pr["n"], bool)
    mask[got["inliers"]] = True
    keep = r["hyp"][got["best_iter"]]["margin"] >= O.NEAR
    assert np.array_equal(mask[keep], pr["planted_inlier"][keep])
    dR, dt = planted_pose_error(pr, got["rt6"])
    assert dR <= POSE_BARS[0] and dt <= POSE_BARS[1]
