"""What a run of the map initialiser (host form or device) must share with the oracle: used by tests/test_mapinit_host.py and
tests/test_mapinit.py."""
import numpy as np

import mapinit_oracle as O


def assert_agrees_with_oracle(h, r, name):
    """what a run (host or device) must share with the oracle; the scenes have no band case and no exempt hypothesis at a winner"""
    for k in ("ok", "model", "winner", "best_h", "best_f", "n_candidates", "n_inliers"):
        assert h[k] == r[k], (name, k, h[k], r[k])
    assert np.array_equal(h["n_good"], r["n_good"]), (name, h["n_good"], r["n_good"])
    assert np.array_equal(h["state"], r["state"]) and np.array_equal(h["matches"], r["matches"])
    assert np.array_equal(h["triangulated"], r["triangulated"])
    if r["model"] != O.NONE:
        # float32 scores of up to 2000 terms each: the terms agree to a few ulps of 5.991 where the models differ in their last bit
        assert abs(h["score_h"] - r["score_h"]) <= 1e-4 * max(r["score_h"], 1) and abs(h["score_f"] - r["score_f"]) <= 1e-4 * max(r["score_f"], 1)
        assert np.allclose(h["parallax"], r["parallax"], rtol=1e-4, atol=1e-4)
    if r["ok"]:
        # R, t come from the float32 model through two SVDs: agreement to a few hundred ulps; the points add the triangulation's
        # conditioning 1 / parallax (3 degrees = 0.05 rad at the least here)
        assert np.abs(h["R"] - r["R"]).max() < 1e-4 and np.abs(h["t"] - r["t"]).max() < 1e-4
        assert np.abs(h["pose"] - r["pose"]).max() < 1e-4
        assert np.allclose(h["points"], r["points"], rtol=2e-3, atol=1e-4)


def assert_planted_non_finite(h, sc, r):
    """what a planted reconstruction (host or device) must share with the oracle's, and what the scene was built for"""
    m = sc["matches"]
    assert r["ok"] == 1 and r["state"][128] == O.NON_FINITE and r["state"][50] == O.NON_FINITE and (r["state"] == O.NON_FINITE).sum() == 2
    assert r["state"][0] == O.COUNTED_GOOD and not r["triangulated"][m[0, 0]]          # set by match 0, cleared by match 128
    assert not r["checks"][r["winner"]]["band"].any()
    for k in ("ok", "model", "winner", "n_candidates", "n_inliers"):
        assert h[k] == r[k], (k, h[k], r[k])
    assert np.array_equal(h["n_good"], r["n_good"]) and np.array_equal(h["state"], r["state"])
    assert np.array_equal(h["triangulated"], r["triangulated"]) and np.array_equal(h["matches"], r["matches"])
    assert np.array_equal(m[h["index"]], h["matches"]) and 0 not in h["index"] and 128 not in h["index"] and 50 not in h["index"]
    assert np.abs(h["R"] - r["R"]).max() < 1e-4 and np.abs(h["t"] - r["t"]).max() < 1e-4
    assert np.allclose(h["points"], r["points"], rtol=2e-3, atol=1e-4) and np.isfinite(h["points"]).all() and np.isfinite(h["p3d"]).all()
