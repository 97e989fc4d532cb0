"""Bundle adjustment with marker observations and free marker poses (uh_ba_set_problem_markers; GlobalOptimizerG2O with map markers,
globaloptimizer_g2o.cpp:156-171, 277-352, 451-455, 526-527): the HIP optimiser against the real g2o (fixture
tests/golden/ba_marker_golden.npz, every case screened against the reference's own float-rounding discontinuities, see
tests/golden/make_ba_marker_golden.py), the marker-free identity, the argument checks, the stop flag and back-to-back problems (gpu);
the fixture's inputs, the cases it covers, its regeneration, the ABI structs and csrc/marker_edge.hpp evaluated on the host (CPU)."""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np
import pytest

import ba_marker_synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "ba_marker_golden.npz")
CASES = ba_marker_synth.CASES
# the project's BA tolerances (tests/test_ba_stereo.py)
STATE_TOL, CHI2_TOL, POINT_TOL, POSE_TOL = 1e-6, 1e-6, 1e-4, 1e-5
JAC_TOL = 1e-6   # agreeing float projections give identical differences; one rounding that falls the other way shows as ~0.1

_problems = {}


def _gen():
    spec = importlib.util.spec_from_file_location("make_ba_marker_golden", os.path.join(HERE, "golden", "make_ba_marker_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _golden():
    return np.load(GOLDEN)


def _problem(name):
    if name not in _problems:
        _problems[name] = ba_marker_synth.marker_ba_problem(**CASES[name])
    return _problems[name]


def _markers(pr):
    return dict(pose_g2m=pr["mk_pose"], size=pr["mk_size"], edge_marker=pr["me_marker"], edge_frame=pr["me_frame"], und_corners=pr["me_corners"],
                edge_weight=pr["me_weight"])


# ------------------------------------------------------------------------------------------------ CPU
def test_problem_generator_reproduces_fixture_inputs():
    g, gen = _golden(), _gen()
    for name in CASES:
        pr = _problem(name)
        np.testing.assert_array_equal(gen.input_digest(pr), g[f"{name}_in_digest"], err_msg=name)
        assert g[f"{name}_state"].shape == (pr["K"], 7) and g[f"{name}_marker_state"].shape == (pr["M"], 7)
        assert g[f"{name}_chi2"].shape == (pr["E"],) and g[f"{name}_marker_chi2"].shape == (pr["EM"],)
        assert g[f"{name}_lin_err"].shape == (pr["EM"], 8) and g[f"{name}_lin_Ji"].shape == (pr["EM"], 8, 6) and g[f"{name}_lin_Jj"].shape == (pr["EM"], 8, 6)


def test_fixture_covers_the_cases():
    g = _golden()
    assert list(CASES) == ["mk_single", "mk_multi", "mk_weights", "mk_only", "mk_stereo", "mk_hard", "mk_wide"]
    pr = {n: _problem(n) for n in CASES}
    free = {n: pr[n]["fixed"][pr[n]["me_frame"]] == 0 for n in CASES}

    def frames_of(p, m):
        return p["me_frame"][p["me_marker"] == m]

    # mk_single: 4 keyframes (1 fixed) x 120 landmarks drawn, one marker seen by two free frames and a fixed one
    p = pr["mk_single"]
    assert (p["K"], int(p["fixed"].sum()), CASES["mk_single"]["P"], p["M"]) == (4, 1, 120, 1)
    assert int(free["mk_single"].sum()) == 2 and int((~free["mk_single"]).sum()) == 1
    assert np.abs(g["mk_single_lin_Jj"][~free["mk_single"]]).max() == 0 and np.abs(g["mk_single_lin_Jj"][free["mk_single"]]).max() > 0
    # mk_multi / mk_hard: 6 x 300, 3 markers seen by 2-5 frames, one of them by fixed frames only, one frame without any landmark
    for n in ("mk_multi", "mk_hard"):
        p = pr[n]
        assert (p["K"], CASES[n]["P"], p["M"]) == (6, 300, 3)
        counts = sorted(len(frames_of(p, m)) for m in range(3))
        assert counts[0] >= 2 and counts[-1] == 5
        assert sum(bool(p["fixed"][frames_of(p, m)].all()) for m in range(3)) == 1
        lonely = np.setdiff1d(np.arange(p["K"]), p["obs_kf"])
        assert len(lonely) == 1 and p["fixed"][lonely[0]] and (p["me_frame"] == lonely[0]).any()
        assert max(np.bincount(p["me_frame"][free[n]])) >= 2   # several edges in one frame block
    # mk_weights: 5 x 150, a frame with kpw <= 40 (weight 1) beside computed weights, a marker without a valid pose counted, unequal cameras
    p = pr["mk_weights"]
    assert (p["K"], CASES["mk_weights"]["P"]) == (5, 150)
    thin = CASES["mk_weights"]["thin_frame"][0]
    assert p["frame_kpw"][thin] <= 40 and (p["me_weight"][p["me_frame"] == thin] == 1.0).all() and (p["me_frame"] == thin).any()
    assert (p["me_weight"][p["me_frame"] != thin] != 1.0).all()
    assert (p["frame_n_markers"] > np.bincount(p["me_frame"], minlength=p["K"])).any()
    assert len(np.unique(p["intr"], axis=0)) == p["K"]
    # mk_only: 5 frames, 4 markers, no landmark at all
    p = pr["mk_only"]
    assert (p["K"], p["M"], p["P"], p["E"]) == (5, 4, 0, 0) and (p["me_weight"] == 1.0).all()
    # mk_stereo: 6 x 300 with about half the observations carrying depth, 2 markers
    p = pr["mk_stereo"]
    assert (p["K"], CASES["mk_stereo"]["P"], p["M"]) == (6, 300, 2) and 0.35 < (p["obs_depth"] > 0).mean() < 0.65
    # mk_hard: Levenberg-Marquardt rejects trials (more trials than iterations); the other cases end passes before their budget
    assert (g["mk_hard_trials"] > g["mk_hard_iters"]).any()
    assert all((g[f"{n}_trials"] == g[f"{n}_iters"]).all() for n in CASES if n != "mk_hard")
    assert sum(g[f"{n}_iters"].tolist() != [5, 10] for n in CASES) >= 5
    # mk_wide: 66 keyframes (65 free) x 200, 5 markers: n = 6 * 70 = 420, several 64-column panels, the marker rows in the last ones
    p = pr["mk_wide"]
    assert (p["K"], int(p["fixed"].sum()), CASES["mk_wide"]["P"], p["M"]) == (66, 1, 200, 5)
    assert 6 * (65 + 5) == 420 and 6 * 65 > 6 * 64
    for n in CASES:
        assert np.isfinite(g[f"{n}_state"]).all() and np.isfinite(g[f"{n}_marker_state"]).all() and np.isfinite(g[f"{n}_marker_chi2"]).all()
        assert len(set(zip(pr[n]["me_marker"].tolist(), pr[n]["me_frame"].tolist()))) == pr[n]["EM"]


def test_weights_follow_the_reference_rule():
    """frame_MarkerWeight (:281-299) on the fixture's own inputs, written out once more."""
    for n in CASES:
        p = _problem(n)
        for e in range(p["EM"]):
            k = p["me_frame"][e]
            sel = p["obs_kf"] == k
            kpw = float(sum(float(np.float32(3.0 if d > 0 else 2.0) * np.float32(w)) for w, d in zip(p["obs_w"][sel], p["obs_depth"][sel])))
            nm = int(p["frame_n_markers"][k])
            want = 1.0
            if kpw > 40 and nm > 0:
                want = (float(np.float32(0.5)) * min(1.0, nm / 5) * kpw) / float(nm * 8)
            assert p["me_weight"][e] == want, (n, e)


def test_driver_regenerates_fixture_bit_for_bit_and_every_case_passes_the_screens():
    gen = _gen()
    why = gen.driver_available()
    if why is not None:
        pytest.skip(why)
    g = _golden()
    new = gen.generate()   # (asserts the conditions for every case and the cap on replaced seeds)
    assert sorted(new) == sorted(g.files)
    for k in g.files:
        np.testing.assert_array_equal(np.asarray(new[k]), g[k], err_msg=k)


def test_marker_abi_struct_layout_and_entries():
    """uh_ba_markers as the Python wrapper declares it = the header's layout on LP64; the existing structs keep their size."""
    import inspect
    import re

    from ucoslam_cv3_amd import ba

    hdr = open(os.path.join(ROOT, "include", "ucoslam_hip.h")).read()
    body = re.search(r"typedef struct uh_ba_markers \{(.*?)\} uh_ba_markers;", hdr, re.S).group(1)
    names = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [f[0] for f in ba._Markers._fields_] == ["n_markers", "pose_g2m", "size", "n_edges", "edge_marker", "edge_frame", "und_corners", "edge_weight"]
    assert C.sizeof(ba._Markers) == 64
    assert [getattr(ba._Markers, n).offset for n in names] == [0, 8, 16, 24, 32, 40, 48, 56]
    assert C.sizeof(ba._Stereo) == 32 and C.sizeof(ba._Problem) == 80 and C.sizeof(ba._Staging) == 56
    for sym in ("uh_ba_set_problem_markers", "uh_ba_get_marker_results"):
        assert re.search(r"\bint\s+" + sym + r"\s*\(", hdr), sym
    assert "markers" in inspect.signature(ba.GlobalOptimizer.setParams).parameters and hasattr(ba.GlobalOptimizer, "getMarkerResults")


_HOST_PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <vector>
#define __host__
#define __device__
#define __forceinline__ inline
#include "marker_edge.hpp"
// per edge in: marker pose 4x4, frame pose 4x4, size, fx fy cx cy, 8 corners, frame free (46 doubles); out: 8 errors, Ji 8x6, Jj 8x6
int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<double> in;
    double v;
    while (fread(&v, 8, 1, f) == 1) in.push_back(v);
    fclose(f);
    const size_t n = in.size() / 46;
    std::vector<double> out(n * 104);
    for (size_t e = 0; e < n; e++) {
        const double* r = &in[46 * e];
        double pose[2][7];
        for (int i = 0; i < 2; i++) {   // toSE3Quat: float 4x4 -> double R, t -> normalised quaternion
            const double* M = r + 16 * i;
            const double R[9] = {M[0], M[1], M[2], M[4], M[5], M[6], M[8], M[9], M[10]};
            quat_from_R(R, pose[i]);
            quat_norm_pos(pose[i]);
            pose[i][4] = M[3]; pose[i][5] = M[7]; pose[i][6] = M[11];
        }
        const double half = marker_half((float)r[32]);
        const bool frame_free = r[45] != 0;
        double err[25][8];
        for (int k = 0; k < 25; k++) {
            double T[7];
            mk_edge_transform(k, pose[0], pose[1], T);
            for (int c = 0; c < 4; c++) mk_corner_error(T, c, half, r + 33, r[37 + 2 * c], r[38 + 2 * c], err[k][2 * c], err[k][2 * c + 1]);
        }
        double* o = &out[104 * e];
        for (int i = 0; i < 8; i++) o[i] = err[0][i];
        for (int row = 0; row < 8; row++)
            for (int d = 0; d < 6; d++) { o[8 + 6 * row + d] = mk_jac(err, 1, d, row); o[56 + 6 * row + d] = frame_free ? mk_jac(err, 13, d, row) : 0.0; }
        // the blocks are what their definition says of these Jacobians
        const double w = 1.75;
        for (int a = 0; a < 6; a++)
            for (int c = 0; c < 6; c++) {
                double mm = 0, mf = 0;
                for (int row = 0; row < 8; row++) { mm += (o[8 + 6 * row + a] * w) * o[8 + 6 * row + c]; mf += (o[8 + 6 * row + a] * w) * o[56 + 6 * row + c]; }
                if (mk_block_entry(err, w, frame_free, 6 * a + c) != mm || mk_block_entry(err, w, frame_free, 84 + 6 * a + c) != mf) return 3;
            }
    }
    f = fopen(argv[2], "wb");
    fwrite(out.data(), 8, out.size(), f);
    fclose(f);
    // the two coefficients of SE3Quat::exp at theta = delta, against this host's libm
    if (kMkDelta != (double)1e-4f || kMkSinc != std::sin(kMkDelta) / kMkDelta || kMkCosc != (1 - std::cos(kMkDelta)) / (kMkDelta * kMkDelta)) return 4;
    return 0;
}
"""


def test_marker_edge_header_on_the_host_matches_g2o_first_linearisation(tmp_path):
    """csrc/marker_edge.hpp compiled for the host: every marker edge of every case at the initial state.  The 8 errors equal the
    fixture's exactly, both Jacobians agree within 1e-6 — what finds a wrong exp, multiplication order or delta before any GPU run."""
    src = tmp_path / "marker_edge_host.cpp"
    src.write_text(_HOST_PROGRAM)
    exe = tmp_path / "marker_edge_host"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "ucoslam-cv3_amd", "csrc"), str(src), "-o", str(exe)])
    g = _golden()
    for name in CASES:
        pr = _problem(name)
        rows = []
        for e in range(pr["EM"]):
            m, k = pr["me_marker"][e], pr["me_frame"][e]
            rows.append(np.concatenate([pr["mk_pose"][m], pr["poses"][k], [pr["mk_size"][m]], pr["intr"][k], pr["me_corners"][e],
                                        [0.0 if pr["fixed"][k] else 1.0]]).astype(np.float64))
        np.stack(rows).tofile(str(tmp_path / "in.bin"))
        subprocess.check_call([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
        o = np.fromfile(str(tmp_path / "out.bin")).reshape(-1, 104)
        dji = np.abs(o[:, 8:56].reshape(-1, 8, 6) - g[f"{name}_lin_Ji"]).max()
        djj = np.abs(o[:, 56:].reshape(-1, 8, 6) - g[f"{name}_lin_Jj"]).max()
        print(name, "edges", pr["EM"], "max |dJi|", dji, "max |dJj|", djj)
        np.testing.assert_array_equal(o[:, :8], g[f"{name}_lin_err"], err_msg=name)
        assert dji < JAC_TOL and djj < JAC_TOL, name


# ------------------------------------------------------------------------------------------------ GPU
def _opt(ctx):
    from ucoslam_cv3_amd.ba import GlobalOptimizer

    return GlobalOptimizer.create(ctx)


def _params():
    from ucoslam_cv3_amd.ba import ParamSet

    return ParamSet(nIters=5)


def _run(opt, pr, markers=True, stop=None):
    stereo = True if (pr["obs_depth"] > 0).any() else None
    opt.setParams(pr, _params(), stereo=stereo, markers=_markers(pr) if markers else None)
    form = opt.form()
    opt.optimize(stop)
    out = opt.getResults()
    out["form"] = form
    if markers:
        out["markers"] = opt.getMarkerResults()
    return out


def _bytes(out):
    b = b"".join(out[k].tobytes() for k in ("poses", "points", "chi2", "bad", "iters", "state"))
    if "markers" in out:
        b += b"".join(out["markers"][k].tobytes() for k in ("poses", "state", "chi2"))
    return b


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_hip_ba_markers_match_real_g2o(hip_ctx, name):
    """Observed on MI355X (max over the seven cases): |state - ref| 2.1e-11, |marker state - ref| 4.3e-11, chi2 6.9e-09 (1 + max) — all
    three in mk_stereo / mk_hard —, float points, poses and marker poses equal to the last bit but one pose entry (5.7e-14);
    iterations and bad flags equal."""
    g = _golden()
    pr = _problem(name)
    got = _run(_opt(hip_ctx), pr)
    mk = got["markers"]
    ref_chi = np.concatenate([g[f"{name}_chi2"], g[f"{name}_marker_chi2"]])
    d = dict(state=np.abs(got["state"] - g[f"{name}_state"]).max(), marker_state=np.abs(mk["state"] - g[f"{name}_marker_state"]).max(),
             chi2=np.abs(np.concatenate([got["chi2"], mk["chi2"]]) - ref_chi).max() / (1 + np.abs(ref_chi).max()),
             points=np.abs(got["points"] - g[f"{name}_points"]).max() if pr["P"] else 0.0, poses=np.abs(got["poses"] - g[f"{name}_poses"]).max(),
             marker_poses=np.abs(mk["poses"] - g[f"{name}_marker_poses"]).max())
    print(name, "form", got["form"], "iters", got["iters"].tolist(), g[f"{name}_iters"].tolist(), " ".join(f"{k} {v:.3g}" for k, v in d.items()))
    assert got["form"] == "wide"
    assert got["iters"].tolist() == g[f"{name}_iters"].tolist()
    assert d["state"] < STATE_TOL and d["marker_state"] < STATE_TOL
    assert d["chi2"] < CHI2_TOL
    assert d["points"] < POINT_TOL
    assert d["poses"] < POSE_TOL and d["marker_poses"] < POSE_TOL
    np.testing.assert_array_equal(got["bad"], g[f"{name}_bad"])


@pytest.mark.gpu
def test_hip_ba_without_marker_edges_is_the_marker_free_problem_bit_for_bit(hip_ctx):
    """markers=None and n_edges = 0 against setParams without markers, on mk_multi's landmarks, in the form that problem takes today."""
    pr = _problem("mk_multi")
    opt = _opt(hip_ctx)
    base = _run(opt, pr, markers=False)
    assert base["form"] != "wide"
    empty = dict(pose_g2m=pr["mk_pose"], size=pr["mk_size"], edge_marker=np.zeros(0, np.int32), edge_frame=np.zeros(0, np.int32),
                 und_corners=np.zeros((0, 8), np.float32), edge_weight=np.zeros(0, np.float64))
    opt.setParams(pr, _params(), markers=empty)
    assert opt.form() == base["form"]
    opt.optimize()
    assert _bytes(opt.getResults()) == _bytes(base)
    import ucoslam_cv3_amd as u
    from ucoslam_cv3_amd._lib import check, lib

    with pytest.raises((RuntimeError, u.UcoslamHipError)):
        opt.getMarkerResults()
    prs, keep, _ = opt._problem_struct(pr)
    check(lib().uh_ba_set_problem_markers(opt._h, C.byref(prs), None, None, C.byref(_params())))   # markers == NULL
    assert opt.form() == base["form"]
    opt.optimize()
    assert _bytes(opt.getResults()) == _bytes(base)


@pytest.mark.gpu
def test_hip_ba_markers_refuse_bad_arguments(hip_ctx):
    import ucoslam_cv3_amd as u
    from ucoslam_cv3_amd import ba
    from ucoslam_cv3_amd._lib import lib, np_ptr

    pr = _problem("mk_single")
    opt = _opt(hip_ctx)
    prs, keep, _ = opt._problem_struct(pr)
    good = {k: np.array(v) for k, v in _markers(pr).items()}
    L = lib()

    def call(m, fields=None):
        ms, keep_m, _ = ba.GlobalOptimizer._markers_struct(m)
        for k, v in (fields or {}).items():
            setattr(ms, k, v)
        rc = L.uh_ba_set_problem_markers(opt._h, C.byref(prs), None, C.byref(ms), C.byref(_params()))
        return rc, (L.uh_last_error() or b"").decode()

    from ucoslam_cv3_amd._lib import UH_EINVAL as einval

    assert call(good)[0] == 0   # the complete call succeeds
    bad = []
    for key, idx, val in (("edge_marker", 0, 1), ("edge_marker", 1, -1), ("edge_frame", 2, pr["K"]), ("edge_frame", 0, -1),
                          ("edge_weight", 1, 0.0), ("edge_weight", 1, -2.0), ("edge_weight", 0, np.nan), ("edge_weight", 2, np.inf),
                          ("size", 0, 0.0), ("size", 0, -0.1), ("size", 0, np.nan), ("size", 0, np.inf)):
        m = {k: v.copy() for k, v in good.items()}
        m[key][idx] = val
        bad.append((f"{key}[{idx}] = {val}", call(m)))
    m = {k: v.copy() for k, v in good.items()}
    m["edge_frame"][1] = m["edge_frame"][0]   # the same (marker, frame) pair twice
    bad.append(("pair twice", call(m)))
    for field in ("pose_g2m", "size", "edge_marker", "edge_frame", "und_corners", "edge_weight"):
        bad.append((f"NULL {field}", call(good, {field: None})))
    bad.append(("n_markers = 0", call(good, {"n_markers": 0})))
    bad.append(("n_edges < 0", call(good, {"n_edges": -1})))
    for what, (rc, msg) in bad:
        assert rc == einval and "uh_ba_set_problem_markers" in msg, (what, rc, msg)
    assert L.uh_ba_set_problem_markers(None, C.byref(prs), None, None, None) == einval
    with pytest.raises(u.UcoslamHipError):   # a refused problem leaves none set
        opt.optimize()
    # the results view refuses, as for every wide problem
    got = _run(opt, pr)
    assert got["form"] == "wide"
    with pytest.raises(u.UcoslamHipError):
        opt.resultsView()


@pytest.mark.gpu
def test_hip_ba_markers_stop_flag_raised_before_optimize(hip_ctx):
    pr = _problem("mk_multi")
    got = _run(_opt(hip_ctx), pr, stop=np.ones(1, np.uint8))
    assert got["iters"].tolist() == [0, 0]
    assert np.abs(got["poses"] - pr["poses"]).max() < 1e-6
    assert np.abs(got["markers"]["poses"] - pr["mk_pose"]).max() < 1e-6
    np.testing.assert_array_equal(got["points"], pr["points"])


@pytest.mark.gpu
def test_hip_ba_marker_problems_back_to_back_are_independent(hip_ctx):
    """A marker problem, a marker-free one, the first again on one optimiser: equal bytes."""
    opt = _opt(hip_ctx)
    a, b = _problem("mk_multi"), _problem("mk_single")
    first = _run(opt, a)
    free = _run(opt, b, markers=False)
    again = _run(opt, a)
    assert first["form"] == "wide" and free["form"] != "wide"
    assert _bytes(again) == _bytes(first)
    assert _bytes(_run(_opt(hip_ctx), b, markers=False)) == _bytes(free)
