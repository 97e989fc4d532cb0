"""The pose-graph fixture and the ABI's argument checks, without a GPU: tests/posegraph_synth.py hashes to the digests in
tests/golden/posegraph_golden.npz, the fixture meets the admission conditions of tests/golden/make_posegraph_golden.py and covers the
cases the optimiser can go wrong at, `--check` reproduces it where the real g2o is built, and uh_posegraph_check_problem (what
uh_posegraph_optimize runs before it launches anything) refuses what the header says it refuses."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import posegraph_synth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "posegraph_golden.npz")
CASES = posegraph_synth.CASES


def _gen():
    spec = importlib.util.spec_from_file_location("make_posegraph_golden", os.path.join(HERE, "golden", "make_posegraph_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_problem_generator_reproduces_fixture_inputs():
    g, gen = np.load(GOLDEN), _gen()
    for name, kw in CASES.items():
        pr = posegraph_synth.posegraph_problem(**kw)
        np.testing.assert_array_equal(gen.input_digest(pr), g[f"{name}_in_digest"], err_msg=name)
        for tag in ("d4", "ref"):
            assert g[f"{name}_{tag}_state"].shape == (pr["n"], 8) and g[f"{name}_{tag}_poses"].shape == (pr["n"], 16)
        assert g[f"{name}_d4_lin_err"].shape == (pr["E"], 7) and g[f"{name}_d4_lin_Ji"].shape == (pr["E"], 7, 7) and g[f"{name}_d4_meas"].shape == (pr["E"], 8)


def test_fixture_meets_the_admission_conditions():
    g, gen = np.load(GOLDEN), _gen()
    assert (gen.SCREEN_TOL, gen.REF_TOL, float(gen.STEPS["d4"]), float(gen.STEPS["ref"])) == (1e-8, 1e-4, float(np.float32(1e-4)), 0.0)
    for name, kw in CASES.items():
        assert float(g[f"{name}_d4_spread_state"]) <= gen.SCREEN_TOL, name
        assert float(g[f"{name}_ref_spread_state"]) <= gen.REF_TOL, name
        assert kw["fix_scale"] or kw["n"] <= 64, name
        for tag in ("d4", "ref"):
            assert np.isfinite(g[f"{name}_{tag}_state"]).all() and np.isfinite(g[f"{name}_{tag}_info"]).all()
            assert 1 <= int(g[f"{name}_{tag}_iters"][0]) < gen.MAX_ITERS   # every case stops through the float chi2 test, none on the budget
    replaced = [n for n, kw in CASES.items() if kw["seed"] != posegraph_synth.FIRST_CHOICE[n]]
    assert 3 * len(replaced) <= len(CASES), replaced
    assert os.path.getsize(GOLDEN) < 512 * 1024


def test_fixture_covers_the_cases():
    g = np.load(GOLDEN)
    pr = {n: posegraph_synth.posegraph_problem(**kw) for n, kw in CASES.items()}
    # two poses, the closing edge only, expected == current: chi2 exactly 0, rho == 0, one iteration with one (rejected) trial
    p = pr["pg2_zero"]
    assert (p["n"], p["E"]) == (2, 1) and np.array_equal(p["expected"], p["poses"][p["idx_new"]])
    for tag in ("d4", "ref"):
        assert g[f"pg2_zero_{tag}_info"][1] == 0 and g[f"pg2_zero_{tag}_info"][2] == 0 and g[f"pg2_zero_{tag}_iters"][0] == 1
    # idx_old in the middle of the index range, idx_new not the last index
    for n in ("pg3", "pg4", "pg5"):
        p = pr[n]
        assert p["n"] == int(n[2:]) and 0 < p["idx_old"] and p["idx_new"] != p["n"] - 1 and p["idx_old"] == p["n"] // 2
    assert pr["pg5"]["idx_old"] < pr["pg5"]["n"] - 1
    # reversed, duplicated and weighted edges
    for n in ("pg8_mixed", "pg12_mixed"):
        p = pr[n]
        pairs = list(zip(p["edge_i"].tolist(), p["edge_j"].tolist()))
        und = [tuple(sorted(q)) for q in pairs]
        assert len(set(und)) < len(und)                                   # a pair occurs twice
        assert any((b, a) in pairs for a, b in pairs)                     # ... once in each order
        assert set(np.unique(p["edge_w"]).tolist()) <= {np.float32(0.2 * 2 ** k) for k in range(5)} and len(np.unique(p["edge_w"])) >= 3
        assert float(p["edge_w"].min()) >= 0.2 - 1e-6 and float(p["edge_w"].max()) <= 3.2 + 1e-6
    assert (pr["pg8_mixed"]["n"], pr["pg12_mixed"]["n"]) == (8, 12)
    # a pose without edges; the old keyframe with several edges
    p = pr["pg12_mixed"]
    assert p["isolated"] >= 0 and p["isolated"] not in p["edge_i"] and p["isolated"] not in p["edge_j"]
    assert int((p["edge_i"] == p["idx_old"]).sum() + (p["edge_j"] == p["idx_old"]).sum()) >= 4
    # rotations above 0.1 rad between keyframes and at the closing edge, a scale jump that moves the scales by several per cent
    m = g["pg12_big_d4_meas"]
    ang = 2 * np.arccos(np.clip(np.abs(m[:, 3]) / np.linalg.norm(m[:, :4], axis=1), 0, 1))
    assert ang.min() > 0.1
    e0 = g["pg12_big_d4_lin_err"]
    assert np.linalg.norm(e0[:, :3], axis=1).max() > 0.1                  # the closing edge's rotation error: log()'s acos branch
    assert np.abs(g["pg12_big_d4_state"][:, 7] - 1).max() > 0.02         # the scales move: the general-sigma branches
    # both sides of the panel width, then several panels
    free = {n: len(set(pr[n]["edge_i"].tolist()) | set(pr[n]["edge_j"].tolist())) - 1 for n in CASES}
    assert (7 * free["pg10"], 7 * free["pg11"], 7 * free["pg20"]) == (63, 70, 133)
    assert 7 * free["pg64_free"] == 441 and 7 * free["pg64_fixed"] == 441 and not CASES["pg64_free"]["fix_scale"] and CASES["pg64_fixed"]["fix_scale"]
    assert 7 * free["pg150_fixed"] == 1043 and CASES["pg150_fixed"]["fix_scale"]
    # fixed scale leaves every s at exactly 1 in the reference as well; free scale moves it
    for n, kw in CASES.items():
        if kw["fix_scale"]:
            assert (g[f"{n}_d4_state"][:, 7] == 1).all() and (g[f"{n}_ref_state"][:, 7] == 1).all()
    # a Levenberg trial is rejected somewhere (more trials than iterations)
    assert any(int(g[f"{n}_d4_trials"].sum()) > int(g[f"{n}_d4_iters"][0]) for n in CASES)


def test_check_regenerates_the_fixture():
    gen = _gen()
    why = gen.driver_available()
    if why is not None:
        pytest.skip(why)
    out = subprocess.run([sys.executable, os.path.join(HERE, "golden", "make_posegraph_golden.py"), "--check"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "reproduced" in out.stdout, out.stdout + out.stderr


def test_argument_checks():
    from ucoslam_cv3_amd import posegraph as pgm

    OK, EINVAL, ECAPACITY = 0, -1, -5
    pr = posegraph_synth.posegraph_problem(**CASES["pg5"])
    base = dict(poses=pr["poses"], edge_i=pr["edge_i"], edge_j=pr["edge_j"], edge_weight=None, idx_new=pr["idx_new"], idx_old=pr["idx_old"],
                expected_pose_new=pr["expected"], fix_scale=0)

    def rc(**kw):
        return pgm.check_problem(**{**base, **kw})

    assert rc() == OK
    assert rc(edge_weight=np.full(pr["E"], 0.5, np.float32)) == OK
    assert rc(max_iters=pgm.MAX_ITERS, lambda_init=1e-3, fd_delta=1e-4) == OK
    assert rc(edge_i=[], edge_j=[]) == OK                                  # no edge at all: the round trip
    for bad in (-1, pr["n"]):
        ei = pr["edge_i"].copy(); ei[2] = bad
        ej = pr["edge_j"].copy(); ej[0] = bad
        assert rc(edge_i=ei) == EINVAL and rc(edge_j=ej) == EINVAL
        assert rc(idx_new=bad) == EINVAL and rc(idx_old=bad) == EINVAL
    ei = pr["edge_i"].copy(); ei[1] = pr["edge_j"][1]
    assert rc(edge_i=ei) == EINVAL                                         # i == j
    assert rc(idx_new=pr["idx_old"]) == EINVAL                             # idx_new == idx_old
    w = np.ones(pr["E"], np.float32); w[3] = np.nan
    assert rc(edge_weight=w) == EINVAL
    assert rc(max_iters=pgm.MAX_ITERS + 1) == EINVAL and rc(max_iters=-1) == EINVAL
    assert rc(lambda_init=-1.0) == EINVAL and rc(fd_delta=-1e-4) == EINVAL and rc(fd_delta=float("nan")) == EINVAL
    assert rc(n_poses=0) == EINVAL
    # the cap: 2048 poses pass, 2049 do not
    assert pgm.MAX_POSES == 2048
    big = np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (pgm.MAX_POSES + 1, 1))
    assert rc(poses=big[:-1]) == OK
    assert rc(poses=big) == ECAPACITY
    assert b"2048" in pgm.lib().uh_last_error()
