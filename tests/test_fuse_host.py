"""The fuse search, the part that needs no GPU: the constructed cases of tests/fuse_cases.py are fixed against the oracle ALONE (every
point takes the branch it was built for), then a stand-alone host build of csrc/fuse_math.hpp + fuse_host.hpp (on the ORACLE's kd-tree)
and the library's uh_fuse_search_host are compared with the oracle: best_kp, best_dist and status equal for every point, no tolerance."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fuse_cases as FC
import fuse_oracle as O
from fuse_checks import PROBLEMS, assert_equal_outputs, oracle_result
from ucoslam_cv3_amd import fuse as UF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELPER = os.path.join(ROOT, "tests", "host_helpers", "fuse_host.cpp")


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_cases_take_their_branches_in_the_oracle(name):
    p, r = PROBLEMS[name], oracle_result(name)
    pts = p["points"]
    print(f"{name}: {pts['n']} points, status histogram {np.bincount(r['status'], minlength=6).tolist()}")
    if not p.get("check_expect", True):
        return
    for i, (nm, ex) in enumerate(zip(pts["names"], pts["expect"])):
        assert r["status"][i] == ex[0], (nm, r["status"][i], ex)
        if ex[1] is not None:
            assert r["best_kp"][i] == ex[1], (nm, r["best_kp"][i], ex)


def test_special_cases_are_what_they_claim():
    """Properties of the constructions that the outcome alone does not show."""
    F = np.float32
    for name in ("kp300_general", "kp2000_identity"):
        p, r = PROBLEMS[name], oracle_result(name)
        pts, info = p["points"], r["info"]
        at = {nm: i for i, nm in enumerate(pts["names"])}
        cc = O.camera_center(p["pose"])
        dist = lambda i: F(O.norm3(cc - pts["pos3d"][i]))   # noqa: E731
        i = at["dist_at_min"]
        assert F(0.8) * pts["min_dist"][i] == dist(i) and r["status"][i] == FC.FOUND
        i = at["dist_at_max"]
        assert F(1.2) * pts["max_dist"][i] == dist(i) and r["status"][i] == FC.FOUND
        for k in (1, 2, 3, 5):
            i = at[f"exact_power{k}"]
            assert F(pts["max_dist"][i] / dist(i)) == FC.SCALE[k]
            print(f"{name}: maxd / dist == scale^{k} exactly -> level {info[i]['level']}")
        i = at["tie"]
        d = info[i]["cand_dist"]
        assert sorted(info[i]["cand"]) == [FC.TIE_A, FC.TIE_B] and d[0] == d[1] == 10 and r["best_kp"][i] == info[i]["cand"][0]
        for nm in ("dense", "dense_widened"):
            i = at[nm]
            assert info[i]["n_cand"] == 200 and sorted(info[i]["cand_dist"])[:2] == [7, 7]
            first7 = info[i]["cand"][info[i]["cand_dist"].index(7)]
            assert r["best_kp"][i] == first7 and r["best_dist"][i] == 7
        assert info[at["cos_above_098"]]["view_cos"] > 0.98 > info[at["cos_below_098"]]["view_cos"]
        assert info[at["cos_above_05"]]["view_cos"] > 0.5 and info[at["level0"]]["level"] == 0 and info[at["level_clamped"]]["level"] == FC.N_LEVELS - 1
        assert r["best_dist"][at["thr_equal"]] == FC.MAX_DESC_DIST and r["best_dist"][at["thr_above"]] == O.desc_threshold(FC.MAX_DESC_DIST)
    p, r = PROBLEMS["kp2000_identity"], oracle_result("kp2000_identity")
    at = {nm: i for i, nm in enumerate(p["points"]["names"])}
    assert r["info"][at["on_min_x"]]["p2d"][0] == 0.0 and r["info"][at["on_min_y"]]["p2d"][1] == 0.0


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fuse") / "libfuse_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", "-o", so, HELPER])
    L = C.CDLL(so)
    L.fu_host_search.restype = C.c_int
    return L


def standalone_search(L, p):
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    fr, pts = p["frame"], p["points"]
    k = fr["und_kpts"]
    nk = len(k)
    xy = np.ascontiguousarray(np.stack([k["x"], k["y"]], 1), np.float32) if nk else np.zeros((1, 2), np.float32)
    t = O.FrameKd(fr).kd.export()
    nn = len(t["col"])
    nodes = np.zeros(max(nn, 1), UF_KDNODE)
    for f in ("divlow", "divhigh", "left", "right", "leaf_begin", "leaf_count", "col"):
        nodes[f][:nn] = t[f]
    octv = np.ascontiguousarray(k["octave"], np.int32) if nk else np.zeros(1, np.int32)
    desc = np.ascontiguousarray(fr["desc"], np.uint8) if nk else np.zeros((1, 32), np.uint8)
    cam = np.array([fr["fx"], fr["fy"], fr["cx"], fr["cy"]], np.float32)
    bounds = np.array([*fr["min_xy"], *fr["max_xy"]], np.int32)
    n = pts["n"]
    bk, bd, st = np.full(max(n, 1), -1, np.int32), np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.uint8)
    sf, psf = np.ascontiguousarray(fr["scale_factors"], np.float32), np.ascontiguousarray(p["predict_sf"], np.float32)
    pose = np.ascontiguousarray(p["pose"], np.float32)
    leaf = t["leaf_idx"] if nk else np.zeros(1, np.uint32)
    rc = L.fu_host_search(P(nodes), nn, P(leaf), P(t["root_bbox"]), P(xy), P(octv), P(desc), nk, P(sf), len(sf), P(cam), P(bounds), P(pose), P(psf), len(psf), n,
                          P(pts["pos3d"]), P(pts["normal"]), P(pts["min_dist"]), P(pts["max_dist"]), P(pts["desc"]), P(pts["skip"]), C.c_float(p["th"]), C.c_float(p["widen"]),
                          C.c_float(p["max_desc_dist"]), P(bk), P(bd), P(st))
    assert rc == 0
    return dict(best_kp=bk[:n], best_dist=bd[:n], status=st[:n])


UF_KDNODE = np.dtype([("divlow", "<f4"), ("divhigh", "<f4"), ("left", "<i4"), ("right", "<i4"), ("leaf_begin", "<i4"), ("leaf_count", "<i2"), ("col", "<i2")])


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_standalone_host_build_equals_oracle(host_lib, name):
    p = PROBLEMS[name]
    assert_equal_outputs(standalone_search(host_lib, p), oracle_result(name), p["points"]["names"], name)


def library_search_host(p, skip=True):
    pts = p["points"]
    return UF.search_host(pts, p["frame"], p["pose"], p["predict_sf"], pts["skip"] if skip else None, p["th"], p["widen"], p["max_desc_dist"])


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_search_host_equals_oracle(name):
    p = PROBLEMS[name]
    assert_equal_outputs(library_search_host(p), oracle_result(name), p["points"]["names"], name)


def test_search_host_without_mask():
    p = PROBLEMS["kp300_general"]
    pts = p["points"]
    ref = O.search(pts, p["frame"], p["pose"], p["predict_sf"], None, p["th"], p["widen"], p["max_desc_dist"])
    got = library_search_host(p, skip=False)
    assert_equal_outputs(got, ref, pts["names"], "no mask")
    assert (got["status"] != FC.SKIPPED).all() and got["status"][pts["names"].index("skip_found")] == FC.FOUND


def test_standalone_program_runs_clean_under_sanitizers(tmp_path):
    """The same host code as a program of its own, with AddressSanitizer and UBSan (no GPU, no Python in the process)."""
    exe = str(tmp_path / "fuse_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DFUSE_HOST_MAIN",
                           HELPER, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr


# ---- refusals of the host form (the device form shares the checks: tests/test_fuse.py)
def _refused(p, match, **over):
    from ucoslam_cv3_amd import UcoslamHipError

    q = dict(p)
    q.update(over)
    with pytest.raises(UcoslamHipError, match=match):
        library_search_host(q)


def test_host_form_refusals():
    p = PROBLEMS["kp300_general"]
    sf = p["predict_sf"]
    _refused(p, "predict_n_levels 9 > the target's 8", predict_sf=np.append(sf, np.float32(4.3)))
    _refused(p, "predict_n_levels 1 < 2", predict_sf=sf[:1])
    big = FC.make_frame(4097, 5)
    _refused(p, "4097 keypoints exceed", frame=big)
    fr = dict(p["frame"])
    fr["und_kpts"] = fr["und_kpts"].copy()
    fr["und_kpts"]["octave"][7] = 16
    _refused(p, "octave 16 of keypoint 7", frame=fr)
    fr = dict(p["frame"])
    fr["scale_factors"] = np.ones(17, np.float32)
    _refused(p, "more than 16", frame=fr)
    _refused(p, "widen", widen=0.0)
    # more points than the stated cap (the arrays are not touched before the check)
    from ucoslam_cv3_amd import UcoslamHipError, lib
    from ucoslam_cv3_amd._lib import check
    from ucoslam_cv3_amd.projmatch import _MapPoints

    cap = lib().uh_fuse_max_points()
    f, keep = UF._frame_struct(p["frame"], True)
    with pytest.raises(UcoslamHipError, match=f"{cap + 1} points outside"):
        check(lib().uh_fuse_search_host(C.byref(_MapPoints(cap + 1, None, None, None, None, None, None)), C.byref(f), None, None, 8, None, 2.5, 1.4, 50.0, None, None, None))
