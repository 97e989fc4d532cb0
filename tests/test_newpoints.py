"""New map points on the GPU (uh_newpoints_run through the C ABI) against the numpy oracle tests/newpoints_oracle.py.

Comparison rules: status, n_new, kp_idx, chosen_*, and the CSR arrays must be EQUAL to the oracle's; xyz_cam / xyz_global within 1 ulp of
float32 per coordinate (both sides take the null vector in double, only the last rounding can differ; tests/test_newpoints_host.py shows
that two CPU paths agree to that).  A match whose smallest oracle margin is below 1e-4 is left out, with the points and lists that
depend on it; the share left out is at most 2 % per scene and 0 in every branch and merge case (asserted here and, for the oracle
alone, in the host test).

Status code 2 (fourth component of the null vector exactly 0) has no case: a float A whose double null vector has an exact zero there
cannot be constructed reliably, the branch is reached only through the shared arithmetic of csrc/newpoints_math.hpp."""
import copy

import numpy as np
import pytest

import newpoints_cases as NC
import newpoints_oracle as O
import newpoints_synth as S
from newpoints_oracle import MAX_NEAR_SHARE, NEAR, ulp_diff

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def np_handle(hip_ctx):
    from ucoslam_cv3_amd.newpoints import NewPoints

    h = NewPoints(hip_ctx)
    yield h
    h.close()


@pytest.fixture(scope="module")
def references():
    """The oracle's result per scene, computed once and never modified."""
    out = {}
    for name in S.CASES:
        kf, pairs = S.case(name)
        out[name] = (kf, pairs, O.run(kf, pairs, ratio_factor=S.RATIO_FACTOR))
    return out


def _points(r, pairs):
    """kp_idx -> everything the merge says about it"""
    out = {}
    for i, kp in enumerate(r["kp_idx"].tolist()):
        a, b = r["obs_ptr"][i], r["obs_ptr"][i + 1]
        out[kp] = (int(r["chosen_pair"][i]), int(r["chosen_match"][i]), r["xyz_global"][i], float(r["distance"][i]),
                   r["obs_pair"][a:b].tolist(), r["obs_kpt"][a:b].tolist())
    return out


def compare(got, ref, pairs, max_share):
    n = len(ref["status"])
    assert len(got["status"]) == n and got["xyz_cam"].shape == (n, 3)
    near = ref["margin"] < NEAR
    assert near.sum() <= max_share * n
    keep = ~near
    assert np.array_equal(got["status"][keep], ref["status"][keep])
    assert np.array_equal(np.isnan(got["xyz_cam"][keep]), np.isnan(ref["xyz_cam"][keep]))
    fin = keep & np.isfinite(ref["xyz_cam"]).all(1)
    worst = int(ulp_diff(got["xyz_cam"][fin], ref["xyz_cam"][fin]).max(initial=0))
    print(f"{n} matches, {int(near.sum())} left out, xyz_cam worst {worst} ulp", end="")
    assert worst <= 1
    if not near.any():
        assert got["n_new"] == ref["n_new"]
        for k in ("kp_idx", "chosen_pair", "chosen_match", "obs_ptr", "obs_pair", "obs_kpt", "distance"):
            assert np.array_equal(got[k], ref[k]), k
        worst_g = int(ulp_diff(got["xyz_global"], ref["xyz_global"]).max(initial=0))
    else:
        off = ref["pair_offset"]
        tainted = set()
        for g in np.nonzero(near)[0]:
            j = int(np.searchsorted(off, g, side="right") - 1)
            tainted.add(int(pairs[j]["matches"]["trainIdx"][g - off[j]]))
        pg, pr = _points(got, pairs), _points(ref, pairs)
        assert set(pg) - tainted == set(pr) - tainted
        worst_g = 0
        for kp in set(pr) - tainted:
            assert pg[kp][:2] == pr[kp][:2] and pg[kp][3:] == pr[kp][3:], kp
            worst_g = max(worst_g, int(ulp_diff(pg[kp][2], pr[kp][2]).max()))
        assert np.all(np.diff(got["kp_idx"]) > 0) and got["obs_ptr"][0] == 0 and got["obs_ptr"][-1] == len(got["obs_pair"])
    print(f", xyz_global worst {worst_g} ulp")
    assert worst_g <= 1


@pytest.mark.parametrize("name", list(S.CASES))
def test_scene_against_the_oracle(np_handle, references, name):
    kf, pairs, ref = references[name]
    got = np_handle.run(kf, pairs, ratio_factor=S.RATIO_FACTOR)
    compare(got, ref, pairs, MAX_NEAR_SHARE)


@pytest.mark.parametrize("name", list(NC.BRANCH))
def test_branch_case(np_handle, name):
    build, code = NC.BRANCH[name]
    kf, pairs = build()
    ref = O.run(kf, pairs, ratio_factor=S.RATIO_FACTOR)
    assert ref["status"].tolist() == [code]   # a scene that does not reach its branch fails here
    got = np_handle.run(kf, pairs, ratio_factor=S.RATIO_FACTOR)
    assert got["status"].tolist() == [code]
    compare(got, ref, pairs, 0.0)


@pytest.mark.parametrize("rule", [O.MERGE_SMALLEST_OCTAVE, O.MERGE_LAST])
def test_merge_cases(np_handle, rule):
    kf, pairs, ex = NC.merge_scene()
    ref = O.run(kf, pairs, ratio_factor=S.RATIO_FACTOR, merge_rule=rule)
    got = np_handle.run(kf, pairs, ratio_factor=S.RATIO_FACTOR, merge_rule=rule)
    assert got["kp_idx"].tolist() == ex["kp_idx"]            # keypoint 2 (its only candidate refused) and 4 (unmatched) make no point
    assert got["chosen_pair"].tolist() == (ex["chosen_pair"] if rule == O.MERGE_SMALLEST_OCTAVE else ex["chosen_pair_as_compiled"])
    assert got["obs_pair"].tolist() == ex["obs_pair"] and got["obs_ptr"].tolist() == ex["obs_ptr"]
    compare(got, ref, pairs, 0.0)


def test_large_then_small_on_one_handle(hip_ctx, references):
    """stale tables: the small problem after the large one gives exactly what it gives on a fresh handle"""
    from ucoslam_cv3_amd.newpoints import NewPoints

    kf_s, pairs_s, ref_s = references["empty_pair"]
    fresh = NewPoints(hip_ctx)
    want = fresh.run(kf_s, pairs_s, ratio_factor=S.RATIO_FACTOR)
    fresh.close()
    h = NewPoints(hip_ctx)
    kf_l, pairs_l, _ = references["wide"]
    h.run(kf_l, pairs_l, ratio_factor=S.RATIO_FACTOR)
    got = h.run(kf_s, pairs_s, ratio_factor=S.RATIO_FACTOR)
    h.close()
    for k in want:
        assert np.array_equal(got[k], want[k], equal_nan=True) if isinstance(want[k], np.ndarray) else got[k] == want[k], k
    compare(got, ref_s, pairs_s, MAX_NEAR_SHARE)


def test_two_runs_are_bit_identical(np_handle, references):
    kf, pairs, _ = references["wide"]
    a = np_handle.run(kf, pairs, ratio_factor=S.RATIO_FACTOR)
    b = np_handle.run(kf, pairs, ratio_factor=S.RATIO_FACTOR)
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].tobytes() == b[k].tobytes(), k
        else:
            assert a[k] == b[k], k


def test_no_pairs_and_no_matches(np_handle, references):
    kf, pairs, _ = references["m63"]
    for ps in ([], [dict(pairs[0], matches=pairs[0]["matches"][:0])]):
        r = np_handle.run(kf, ps, ratio_factor=S.RATIO_FACTOR)
        assert r["n_new"] == 0 and len(r["status"]) == 0 and r["obs_ptr"].tolist() == [0]


def _broken(references, what):
    kf, pairs, _ = references["empty_pair"]
    kf, pairs = copy.deepcopy(kf), copy.deepcopy(pairs)
    m = pairs[1]["matches"]
    if what == "queryIdx":
        m["queryIdx"][7] = len(pairs[1]["octave"])
    elif what == "trainIdx":
        m["trainIdx"][7] = len(kf["octave"])
    elif what == "negative trainIdx":
        m["trainIdx"][7] = -1
    elif what == "octave":
        pairs[1]["octave"][m["queryIdx"][7]] = S.N_LEVELS
    elif what == "repeated trainIdx":
        m["trainIdx"][7] = m["trainIdx"][3]
    elif what == "too many keypoints":
        n = 16385
        kf["pt"], kf["octave"] = np.zeros((n, 2), np.float32), np.zeros(n, np.int32)
    return kf, pairs


@pytest.mark.parametrize("what", ["queryIdx", "trainIdx", "negative trainIdx", "octave", "repeated trainIdx", "too many keypoints"])
def test_validation_refuses_before_launch_and_the_handle_survives(np_handle, references, what):
    from ucoslam_cv3_amd import UcoslamHipError
    from ucoslam_cv3_amd._lib import UH_EINVAL

    kf, pairs = _broken(references, what)
    with pytest.raises(UcoslamHipError) as ei:
        np_handle.run(kf, pairs, ratio_factor=S.RATIO_FACTOR)
    assert ei.value.code == UH_EINVAL
    if what != "too many keypoints":
        assert "pair 1 match 7" in str(ei.value)
    kf, pairs, ref = references["empty_pair"]
    compare(np_handle.run(kf, pairs, ratio_factor=S.RATIO_FACTOR), ref, pairs, MAX_NEAR_SHARE)
