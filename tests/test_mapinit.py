"""The map initialiser on the device (uh_mapinit_run) through the C ABI: against the numpy oracle, against uh_mapinit_run_host bit for bit,
and hypothesis by hypothesis through the debug hook.  The scenes are those tests/test_mapinit_host.py fixes against the oracle alone
(shares of exempt hypotheses and band pairs, no winner among them).

Sizes: n in {8, 9, 63, 64, 65, 129, 257, 1000} (mask-word and wave-stride edges; min_matches = 8 for the small ones), keypoint counts
larger than n, iterations in {1, 3, 4, 5, 200}.

Observed on an MI355X: see README (map initialiser, unpinned paragraph) for the worst hypothesis-matrix distance."""
import numpy as np
import pytest

import mapinit_cases as MC
import mapinit_oracle as O
from mapinit_checks import assert_agrees_with_oracle, assert_planted_non_finite

pytestmark = pytest.mark.gpu

BITWISE = ("ok", "model", "winner", "best_h", "best_f", "score_h", "score_f", "rh", "n_candidates", "n_inliers", "n_good", "R", "t", "pose", "matches",
           "points", "triangulated", "p3d", "state", "index")
HOOK_BAR = 1e-6


@pytest.fixture(scope="module")
def mi(hip_ctx):
    from ucoslam_cv3_amd import MapInit

    m = MapInit(hip_ctx)
    yield m
    m.close()


def run(mi, name, **over):
    sc = MC.scene(name)
    return mi.initialize(sc["intr"], sc["kp1"], sc["kp2"], sc["matches"], **dict(sc["kw"], **over))


def assert_bitwise(a, b, what):
    for k in BITWISE:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (what, k, a[k], b[k])


@pytest.mark.parametrize("name", list(MC.SCENES))
def test_device_against_oracle_and_host(mi, name):
    from ucoslam_cv3_amd import initialize_host

    sc, r = MC.scene(name), MC.oracle(name)
    got = run(mi, name)
    assert_agrees_with_oracle(got, r, name)
    host = initialize_host(sc["intr"], sc["kp1"], sc["kp2"], sc["matches"], **sc["kw"])
    assert_bitwise(got, host, name)
    # the parallax alone may differ: acos of the device's library against the host's, both within an ulp or two of the double result,
    # rounded to float once: at most one float ulp of a value below 180
    assert np.abs(got["parallax"] - host["parallax"]).max() <= 180 * np.finfo(np.float32).eps
    if r["ok"]:   # every scene the reference accepts
        bar, err = MC.pose_bar(sc), MC.pose_error(got["R"], got["t"], sc)
        print(f"{name}: pose error {err[0]:.5f} rad / {err[1]:.5f} rad against bars {bar[0]:.5f} / {bar[1]:.5f}")
        assert err[0] <= bar[0] and err[1] <= bar[1]


@pytest.mark.parametrize("name", [k for k in MC.SCENES if k != "n49_defaults"])   # (49 matches run no hypothesis)
def test_every_hypothesis_through_the_hook(mi, name):
    """Each hypothesis' double matrix within 1e-6 of the oracle's after scaling both to unit norm (hypotheses whose system has
    sigma_1 / sigma_8 above 1e8 in the oracle are exempt); masks equal outside the band pairs; scores as close as the terms allow."""
    sc, r = MC.scene(name), MC.oracle(name)
    worst = 0.0
    for m, model in enumerate((O.HOMOGRAPHY, O.FUNDAMENTAL)):
        for it, h in enumerate(r["hyps"][m]):
            d = mi.debug_hypothesis(sc["intr"], sc["kp1"], sc["kp2"], sc["matches"], model, it, samples=r["samples"], iterations=len(r["samples"]),
                                    **{k: v for k, v in sc["kw"].items() if k != "iterations"})
            if h["cond"] > MC.COND_EXEMPT:
                continue
            a, b = d["M"] / np.linalg.norm(d["M"]), h["M"] / np.linalg.norm(h["M"])
            dist = min(np.abs(a - b).max(), np.abs(a + b).max())
            worst = max(worst, dist)
            assert dist <= HOOK_BAR, (name, model, it, dist, h["cond"])
            assert np.array_equal(d["mask"][~h["band"]], h["mask"][~h["band"]]), (name, model, it)
            assert abs(d["score"] - h["score"]) <= 1e-4 * max(h["score"], 1) + 5.991 * 2 * h["band"].sum()
    print(f"{name}: worst distance of a unit-norm hypothesis matrix from the oracle's: {worst:.3e}")


def test_planted_non_finite_triangulation(mi):
    """The second launch alone on a planted winner (uh_mapinit_debug_reconstruct): the non-finite state through the candidates' rows, the
    winner's copy and the host scatter that clears the flag; against the oracle and against the host form bit for bit."""
    from ucoslam_cv3_amd.mapinit import debug_reconstruct_host

    sc, model, M, mask, r = MC.planted_non_finite()
    args = (sc["intr"], sc["kp1"], sc["kp2"], sc["matches"], model, M, mask)
    got = mi.debug_reconstruct(*args)
    assert_planted_non_finite(got, sc, r)
    assert_bitwise(got, debug_reconstruct_host(*args), "planted non-finite")


def test_planted_winner_equals_the_whole_run(mi):
    """The hook runs the launch the whole run runs: planted with the device's own winning matrix and mask it gives the whole run's result"""
    for name in ("duplicates_129", "plane_outliers_257"):
        sc, r = MC.scene(name), MC.oracle(name)
        whole = run(mi, name)
        model, it = whole["model"], whole["best_h"] if whole["model"] == O.HOMOGRAPHY else whole["best_f"]
        d = mi.debug_hypothesis(sc["intr"], sc["kp1"], sc["kp2"], sc["matches"], model, it, **sc["kw"])
        part = mi.debug_reconstruct(sc["intr"], sc["kp1"], sc["kp2"], sc["matches"], model, d["Mf"], d["mask"], **sc["kw"])
        for k in ("ok", "model", "winner", "n_candidates", "n_inliers", "n_good", "parallax", "R", "t", "pose", "matches", "points", "triangulated", "p3d",
                  "state", "index"):
            assert np.asarray(whole[k]).tobytes() == np.asarray(part[k]).tobytes(), (name, k)


def test_given_samples_equal_drawn_samples_and_calls_repeat(mi):
    for name in ("general_1000", "n63_it4"):
        sc = MC.scene(name)
        iters = sc["kw"].get("iterations", 200)
        a = run(mi, name)
        b = run(mi, name, samples=O.draw_samples(len(sc["matches"]), iters))
        c = run(mi, name)
        assert_bitwise(a, b, name + " samples")
        assert_bitwise(a, c, name + " repeat")
        assert a["parallax"].tobytes() == b["parallax"].tobytes() == c["parallax"].tobytes()


def test_short_input_and_refusals(mi):
    from ucoslam_cv3_amd import UcoslamHipError

    got = run(mi, "n49_defaults")
    assert got["ok"] == 0 and got["model"] == O.NONE and len(got["matches"]) == 0
    with pytest.raises(UcoslamHipError):
        run(mi, "n65", min_matches=7)
    sc = MC.scene("n65")
    bad = sc["matches"].copy()
    bad[0, 1] = -1
    with pytest.raises(UcoslamHipError):
        mi.initialize(sc["intr"], sc["kp1"], sc["kp2"], bad, min_matches=8)
    assert run(mi, "n65")["ok"] == 1   # the object is usable after a refusal
