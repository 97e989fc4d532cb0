"""The whole fuse step without a GPU: the toy map of tests/fuse_map_cases.py through the oracle (every event kind occurs; the update path
cannot be skipped unnoticed), through the C++ adaptor ucoslam_hip::MapPointFuser on uh_fuse_search_host (tests/host_helpers/fuse_adaptor.cpp)
and through the Python mirror — the final map equals the oracle's: ids of every keyframe, frames and bad flag of every point, normal,
min / max distance and descriptor bit for bit, and the returned list."""
import collections
import copy
import os
import subprocess

import fuse_map_cases as MC
import fuse_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ucoslam-cv3_amd", "libucoslam_hip.so")
_CACHE = {}


def toy():
    """(entry map, oracle's final map, removed list, log): computed once per session, never modified."""
    if not _CACHE:
        m = MC.scene()
        final = copy.deepcopy(m)
        removed, log = O.search_in_neighbors(final, MC.CUR, MC.MAX_DESC_DIST)
        _CACHE.update(entry=m, final=final, removed=removed, log=log, state=O.map_state(final))
    return _CACHE


def build_adaptor(tmp_path):
    exe = str(tmp_path / "fuse_adaptor")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "host_helpers", "fuse_adaptor.cpp"),
                           "-L", os.path.dirname(LIB), "-lucoslam_hip", f"-Wl,-rpath,{os.path.dirname(LIB)}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def run_adaptor(exe, tmp_path, *form):
    t = toy()
    src, dst = str(tmp_path / "map.bin"), str(tmp_path / "state.bin")
    MC.dump_map(t["entry"], MC.CUR, MC.MAX_DESC_DIST, src)
    out = subprocess.run([exe, src, dst, *form], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "fuse adaptor ok" in out.stdout, out.stdout + out.stderr
    return out.stdout, MC.load_state(t["entry"], dst)


def assert_same_map(removed, state, what):
    t = toy()
    assert removed == t["removed"], what
    diff = [k for k in t["state"] if state.get(k) != t["state"][k]]
    assert not diff and len(state) == len(t["state"]), f"{what}: differs at {diff[:10]}"


def test_every_event_occurs_in_the_oracle():
    t = toy()
    ev, m = t["log"]["events"], t["entry"]
    kinds = collections.Counter((e[0], e[3]) for e in ev)
    print("events (half, kind):", dict(kinds), "removed:", len(t["removed"]), "state-dependent:", len(t["log"]["state_dependent"]))
    assert len(m["map_points"]) == 280 and len(m["keyframes"]) == 6
    assert kinds[(1, "add")] == 300 and kinds[(1, "fuse")] == 60 and kinds[(2, "add")] == 30 and kinds[(2, "fuse")] == 20
    assert t["log"]["targets"] == [3, 5, 7, 8]                                  # the bad neighbour is left out, the order is ascending
    assert not any(e[1] == MC.BAD for e in ev)
    # two points choosing the same free keypoint of one keyframe: the first adds, the second fuses into it
    same = [(a, b) for i, b in enumerate(ev) if b[3] == "fuse" for a in ev[:i] if a[:2] == b[:2] and a[3] == "add" and a[4] == b[4] and b[5] == a[2]]
    assert len(same) == 10
    # a point added in keyframe 3 whose new descriptor and normal decide its outcome in keyframe 5
    dep = t["log"]["state_dependent"]
    assert len(dep) == 10 and all(kf == 5 for kf, _ in dep)
    for kf, pid in dep:
        assert (1, 3, pid, "add") in [e[:4] for e in ev] and (1, 5, pid, "add") in [e[:4] for e in ev]
        e0, e1 = m["map_points"][pid], t["final"]["map_points"][pid]
        assert e0["desc"].tobytes() != e1["desc"].tobytes() and e0["normal"].tobytes() != e1["normal"].tobytes()
    # a fusion target that is itself a point of the new keyframe
    cur_pts = set(int(i) for i in m["keyframes"][MC.CUR]["ids"] if i != O.NO_ID)
    assert sum(1 for e in ev if e[0] == 1 and e[3] == "fuse" and e[5] in cur_pts) >= 10
    # the second half's fusions take their descriptor from the bad keyframe
    assert all(MC.BAD in m["map_points"][e[2]]["frames"] for e in ev if e[:1] == (2,) and e[3] == "fuse")


def test_cpp_adaptor_on_the_host_form_equals_oracle(tmp_path):
    stdout, (removed, state) = run_adaptor(build_adaptor(tmp_path), tmp_path)
    print(stdout)
    assert "(host): 80 removed, 80 of 280 points bad, 830 observations, 0 device frames cached" in stdout
    assert "second call: 0 removed, 869 observations" in stdout
    assert_same_map(removed, state, "MapPointFuser on uh_fuse_search_host")


def test_python_mirror_on_the_host_form_equals_oracle():
    from ucoslam_cv3_amd import search_in_neighbors

    m = copy.deepcopy(toy()["entry"])
    removed = search_in_neighbors(m, MC.CUR, MC.MAX_DESC_DIST)
    assert_same_map(removed, O.map_state(m), "fuse.search_in_neighbors on uh_fuse_search_host")


def test_skipping_the_update_is_noticed():
    """The same composition with the entry records kept for the whole first half (what one batched launch over all targets would compute)
    ends in another map: the parity bar sees a skipped update."""
    from ucoslam_cv3_amd import fuse as UF

    t = toy()
    m = copy.deepcopy(t["entry"])
    real = UF._table
    frozen = {pid: {k: copy.deepcopy(v) for k, v in mp.items()} for pid, mp in t["entry"]["map_points"].items()}
    try:
        UF._table = lambda mm, ids: real(dict(mm, map_points={i: frozen[i] for i in ids if i in frozen}), ids)
        removed = UF.search_in_neighbors(m, MC.CUR, MC.MAX_DESC_DIST)
    finally:
        UF._table = real
    state = O.map_state(m)
    assert removed != t["removed"] or any(state[k] != t["state"][k] for k in state)
