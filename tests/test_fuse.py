"""The fuse search on the device (csrc/fuse.hip): uh_fuse_search against the oracle and against uh_fuse_search_host on every constructed
case of tests/fuse_cases.py — best_kp, best_dist and status equal for every point, bit for bit — with both tree builders of the device
frame, the handle's upload path, the frame outside LDS, row updates, two targets on one handle and every refusal; then the whole function
(tests/fuse_map_cases.py) through the Python mirror and through the C++ adaptor on the device, whose final map equals the oracle's."""
import copy
import os
import subprocess

import numpy as np
import pytest

import fuse_cases as FC
import fuse_oracle as O
from fuse_checks import PROBLEMS, assert_equal_outputs, oracle_result

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fuser(hip_ctx):
    from ucoslam_cv3_amd.fuse import FuseSearch

    f = FuseSearch(hip_ctx)
    yield f
    f.close()


def _set_points(fuser, p):
    pts = p["points"]
    fuser.setPoints(pts["pos3d"], pts["normal"], pts["min_dist"], pts["max_dist"], pts["desc"])


def _dev_frame(hip_ctx, fr, host_tree):
    from ucoslam_cv3_amd.orb import DeviceFrame

    return DeviceFrame(hip_ctx).setTreeBuilder(host_tree).upload(fr["und_kpts"], fr["desc"])


def _search(fuser, p, dev=None, skip=True):
    return fuser.search(p["frame"], p["pose"], p["predict_sf"], dev, p["points"]["skip"] if skip else None, p["th"], p["widen"], p["max_desc_dist"])


@pytest.mark.parametrize("name", list(PROBLEMS))
@pytest.mark.parametrize("frame_form", ["device_tree", "host_tree", "upload"])
def test_search_equals_oracle_and_host_form(hip_ctx, fuser, name, frame_form):
    from ucoslam_cv3_amd.fuse import search_host

    p = PROBLEMS[name]
    pts = p["points"]
    _set_points(fuser, p)
    dev = None if frame_form == "upload" else _dev_frame(hip_ctx, p["frame"], frame_form == "host_tree")
    got = _search(fuser, p, dev)
    assert_equal_outputs(got, oracle_result(name), pts["names"], f"{name} / {frame_form} against the oracle")
    host = search_host(pts, p["frame"], p["pose"], p["predict_sf"], pts["skip"], p["th"], p["widen"], p["max_desc_dist"])
    assert_equal_outputs(got, host, pts["names"], f"{name} / {frame_form} against uh_fuse_search_host")
    if dev is not None:
        dev.close()


@pytest.mark.parametrize("name", ["kp2000_general", "kp300_general"])
def test_frame_outside_lds(hip_ctx, fuser, name, monkeypatch):
    """The kernel's other instantiation: nodes and leaf records read from HBM (what a frame too large for the LDS budget takes)."""
    p = PROBLEMS[name]
    _set_points(fuser, p)
    dev = _dev_frame(hip_ctx, p["frame"], False)
    monkeypatch.setenv("UH_FUSE_NO_LDS", "1")
    got = _search(fuser, p, dev)
    assert_equal_outputs(got, oracle_result(name), p["points"]["names"], f"{name} outside LDS")
    dev.close()


def test_4096_keypoints_and_many_points(hip_ctx, fuser):
    """The largest device frame (4096 keypoints; its tree still fits the LDS budget) under 1500 points — 6 points per workgroup, every
    compute unit busy — against the host form, and 60 of them against the oracle."""
    from ucoslam_cv3_amd.fuse import search_host

    fr = FC.make_frame(4096, 21)
    T = FC.view("general")
    rng = np.random.default_rng(3)
    b = FC._Builder(T)
    k = fr["und_kpts"]
    for i in range(1500):
        j = int(rng.integers(0, 4096))
        b.add(f"p{i}", None, k["x"][j] + rng.uniform(-2, 2), k["y"][j] + rng.uniform(-2, 2), z=rng.uniform(2, 8), level=int(k["octave"][j]) + int(rng.integers(0, 3)),
              angle=rng.uniform(0, 65), desc=FC._flip(fr["desc"][j], rng.choice(256, int(rng.integers(0, 60)), replace=False)))
    pts = FC._table(b.rows)
    fuser.setPoints(pts["pos3d"], pts["normal"], pts["min_dist"], pts["max_dist"], pts["desc"])
    dev = _dev_frame(hip_ctx, fr, False)
    got = fuser.search(fr, T, FC.SCALE, dev, None, 2.5, 1.4, FC.MAX_DESC_DIST)
    host = search_host(pts, fr, T, FC.SCALE, None, 2.5, 1.4, FC.MAX_DESC_DIST)
    assert_equal_outputs(got, host, pts["names"], "4096 keypoints x 1500 points against uh_fuse_search_host")
    hist = np.bincount(got["status"], minlength=6)
    print("status histogram", hist.tolist())
    # by construction: a twelfth of the angles lie past 60 degrees, a third of the levels miss the keypoint's octave, a sixth of the descriptors the threshold
    assert hist[0] > 500 and hist[4] > 60 and hist[5] > 300
    sub = {kk: (v[:60] if isinstance(v, (np.ndarray, list)) else v) for kk, v in pts.items()}
    ref = O.search(sub, fr, T, FC.SCALE, None, 2.5, 1.4, FC.MAX_DESC_DIST)
    assert_equal_outputs({kk: v[:60] for kk, v in got.items()}, ref, pts["names"], "first 60 points against the oracle")
    dev.close()


def test_update_points_changes_only_the_updated_rows(hip_ctx, fuser):
    name = "kp300_general"
    p = PROBLEMS[name]
    pts = p["points"]
    at = {nm: i for i, nm in enumerate(pts["names"])}
    _set_points(fuser, p)
    dev = _dev_frame(hip_ctx, p["frame"], False)
    before = _search(fuser, p, dev)
    # thr_above takes thr_equal's descriptor (found now); level3 takes level6's distances; iso_found moves behind the camera
    rows = [at["thr_above"], at["level3"], at["iso_found"]]
    new = {k: pts[k].copy() for k in ("pos3d", "normal", "min_dist", "max_dist", "desc")}
    new["desc"][rows[0]] = pts["desc"][at["thr_equal"]]
    new["max_dist"][rows[1]], new["min_dist"][rows[1]] = pts["max_dist"][at["level6"]], pts["min_dist"][at["level6"]]
    new["pos3d"][rows[2]] = pts["pos3d"][at["behind"]]
    fuser.updatePoints(rows, *[new[k][rows] for k in ("pos3d", "normal", "min_dist", "max_dist", "desc")])
    after = _search(fuser, p, dev)
    ref = O.search(dict(new, n=pts["n"]), p["frame"], p["pose"], p["predict_sf"], pts["skip"], p["th"], p["widen"], p["max_desc_dist"])
    assert_equal_outputs(after, ref, pts["names"], "after uh_fuse_update_points")
    changed = [i for i in range(pts["n"]) if (before["status"][i], before["best_kp"][i]) != (after["status"][i], after["best_kp"][i])]
    assert sorted(changed) == sorted(rows)
    assert (after["status"][rows[0]], after["best_kp"][rows[0]]) == (FC.FOUND, FC.ISO) and after["best_kp"][rows[1]] == FC.LADDER0 + 6 and after["status"][rows[2]] == FC.NO_PROJECT
    dev.close()


def test_two_targets_in_a_row_on_one_handle(hip_ctx, fuser):
    a, b = PROBLEMS["kp2000_general"], PROBLEMS["kp300_general"]   # (same view, same point list, different frames)
    _set_points(fuser, a)
    da, db = _dev_frame(hip_ctx, a["frame"], False), _dev_frame(hip_ctx, b["frame"], True)
    ra = _search(fuser, a, da)
    rb = _search(fuser, b, db)
    ra2 = _search(fuser, a, da)
    assert_equal_outputs(ra, oracle_result("kp2000_general"), a["points"]["names"], "first target")
    assert_equal_outputs(rb, oracle_result("kp300_general"), b["points"]["names"], "second target")
    assert_equal_outputs(ra2, ra, a["points"]["names"], "first target again")
    da.close(), db.close()


def test_refusals(hip_ctx, fuser):
    from ucoslam_cv3_amd import UcoslamHipError
    from ucoslam_cv3_amd.fuse import FuseSearch
    from ucoslam_cv3_amd.orb import DeviceFrame

    p = PROBLEMS["kp300_general"]
    pts = p["points"]
    fresh = FuseSearch(hip_ctx)
    with pytest.raises(UcoslamHipError, match="no point table"):
        _search(fresh, p, skip=False)
    fresh.close()
    _set_points(fuser, p)
    with pytest.raises(UcoslamHipError, match="predict_n_levels 9 > the target's 8"):
        fuser.search(p["frame"], p["pose"], np.append(p["predict_sf"], np.float32(4.3)), None, None, 2.5, 1.4, 50.0)
    with pytest.raises(UcoslamHipError, match="predict_n_levels 1 < 2"):
        fuser.search(p["frame"], p["pose"], p["predict_sf"][:1], None, None, 2.5, 1.4, 50.0)
    row = {k: pts[k][:1] for k in ("pos3d", "normal", "min_dist", "max_dist", "desc")}
    for bad in (pts["n"], -1):
        with pytest.raises(UcoslamHipError, match=r"rows\[0\] = %d outside the table of %d" % (bad, pts["n"])):
            fuser.updatePoints([bad], *row.values())
    empty = DeviceFrame(hip_ctx)
    with pytest.raises(UcoslamHipError, match="no complete kd-tree"):
        fuser.search(p["frame"], p["pose"], p["predict_sf"], empty, None, 2.5, 1.4, 50.0)
    empty.close()
    with pytest.raises(UcoslamHipError, match="4097 keypoints exceed"):
        fuser.search(FC.make_frame(4097, 5), p["pose"], p["predict_sf"], None, None, 2.5, 1.4, 50.0)
    host_tree = _dev_frame(hip_ctx, p["frame"], True)
    short = dict(p["frame"], und_kpts=p["frame"]["und_kpts"][:100], desc=p["frame"]["desc"][:100])
    with pytest.raises(UcoslamHipError, match="100 keypoints for a device frame of 300"):
        fuser.search(short, p["pose"], p["predict_sf"], host_tree, None, 2.5, 1.4, 50.0)
    host_tree.close()
    # the handle still works after every refusal
    assert_equal_outputs(_search(fuser, p), oracle_result("kp300_general"), pts["names"], "after the refusals")


def test_point_cap(hip_ctx):
    import ctypes as C

    from ucoslam_cv3_amd import UcoslamHipError, lib
    from ucoslam_cv3_amd.fuse import FuseSearch
    from ucoslam_cv3_amd.projmatch import _MapPoints

    f = FuseSearch(hip_ctx)
    cap = lib().uh_fuse_max_points()
    with pytest.raises(UcoslamHipError, match="outside"):
        from ucoslam_cv3_amd._lib import check

        check(lib().uh_fuse_set_points(f._h, C.byref(_MapPoints(cap + 1, None, None, None, None, None, None))))
    f.close()


# ------------------------------------------------------------------------------------------------ the whole function on the device
def test_python_mirror_on_the_device_equals_oracle(hip_ctx):
    import fuse_map_cases as MC
    from test_fuse_adaptor import assert_same_map, toy
    from ucoslam_cv3_amd import FuseSearch, search_in_neighbors
    from ucoslam_cv3_amd.orb import DeviceFrame

    m = copy.deepcopy(toy()["entry"])
    f = FuseSearch(hip_ctx)
    # one resident frame per keyframe of the window, both tree builders among them; keyframe 8 goes through the handle's upload path
    frames = {i: DeviceFrame(hip_ctx).setTreeBuilder(i in (5, MC.CUR)).upload(kf["und_kpts"], kf["desc"]) for i, kf in m["keyframes"].items() if i not in (8, MC.BAD)}
    removed = search_in_neighbors(m, MC.CUR, MC.MAX_DESC_DIST, fuser=f, dev_frames=frames)
    assert_same_map(removed, O.map_state(m), "fuse.search_in_neighbors on the device")
    f.close()
    for d in frames.values():
        d.close()


def test_cpp_adaptor_on_the_device_equals_oracle(tmp_path):
    from test_fuse_adaptor import assert_same_map, build_adaptor, run_adaptor

    stdout, (removed, state) = run_adaptor(build_adaptor(tmp_path), tmp_path, "device")
    print(stdout)
    assert "(device): 80 removed, 80 of 280 points bad" in stdout and "5 device frames cached" in stdout
    assert "second call: 0 removed, 869 observations, 5 device frames cached (5 before)" in stdout   # (as the host form's second call)
    assert_same_map(removed, state, "MapPointFuser on the device")


def test_example_new_points_then_fuse(tmp_path):
    """examples/fuse_points.cpp: NewPointCreator, then MapPointFuser, for one keyframe and three neighbours; the fuse stage on the device and on
    the host form end in the same map counts."""
    import json

    lib_dir = os.path.join(ROOT, "ucoslam-cv3_amd")
    exe = str(tmp_path / "fuse_points")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-o", exe, os.path.join(ROOT, "examples", "fuse_points.cpp"), "-L", lib_dir, "-lucoslam_hip",
                           f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    res = []
    for form in ([], ["host"]):
        out = subprocess.run([exe, *form], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        res.append(json.loads(out.stdout.strip().splitlines()[-1]))
    print(res[0])
    assert res[0]["device_frames"] == 4 and res[1]["device_frames"] == 0
    assert {k: v for k, v in res[0].items() if k != "device_frames"} == {k: v for k, v in res[1].items() if k != "device_frames"}
    assert res[0]["new_points"] > 100 and res[0]["fused_away"] > 20 and res[0]["observations_after"] > res[0]["observations_before"] + 100
