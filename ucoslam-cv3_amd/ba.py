"""Host-side mirror of the reference BA plugin on top of the C ABI.

Reference surface: `GlobalOptimizer` (src/optimization/globaloptimizer.h:28-68): `create(type)`,
`setParams(map, ParamSet)`, `optimize(bool* stopASAP)`, `getResults(map)`, `getBadAssociations()`, `getName()`.
The map is passed already flattened (dict of arrays, see include/ucoslam_hip.h uh_ba_problem).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import I, VP, check, lib, np_ptr


class _Problem(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("n_points", C.c_int32), ("n_obs", C.c_int32), ("poses_f2g", VP), ("fixed", VP),
                ("intr", VP), ("points", VP), ("obs_point", VP), ("obs_frame", VP), ("obs_uv", VP), ("obs_inv_sigma", VP)]


class ParamSet(C.Structure):
    """The subset of GlobalOptimizer::ParamSet that the monocular path uses (globaloptimizer.h:31-47)."""
    _fields_ = [("n_iters", C.c_int32), ("huber_delta", C.c_double), ("chi2_threshold", C.c_double),
                ("min_chi2_between_iter", C.c_float)]

    def __init__(self, nIters=5, huber_delta=0.0, chi2_threshold=0.0, min_chi2_between_iter=1.0):
        super().__init__(nIters, huber_delta, chi2_threshold, min_chi2_between_iter)


class _Staging(C.Structure):
    _fields_ = [("poses_f2g", VP), ("fixed", VP), ("intr", VP), ("points", VP), ("obs", VP),
                ("cap_frames", C.c_int32), ("cap_points", C.c_int32), ("cap_obs", C.c_int32)]


class _Stereo(C.Structure):   # uh_ba_stereo
    _fields_ = [("obs_depth", VP), ("frame_bl", VP), ("huber_delta_3d", C.c_double), ("chi2_threshold_3d", C.c_double)]


class _StagingStereo(C.Structure):   # uh_ba_staging_stereo
    _fields_ = [("poses_f2g", VP), ("fixed", VP), ("intr", VP), ("points", VP), ("obs", VP), ("obs_depth", VP), ("frame_bl", VP),
                ("cap_frames", C.c_int32), ("cap_points", C.c_int32), ("cap_obs", C.c_int32)]


class _Markers(C.Structure):   # uh_ba_markers
    _fields_ = [("n_markers", C.c_int32), ("pose_g2m", VP), ("size", VP), ("n_edges", C.c_int32), ("edge_marker", VP), ("edge_frame", VP),
                ("und_corners", VP), ("edge_weight", VP)]


class _ResultsView(C.Structure):
    _fields_ = [("poses", VP), ("points", VP), ("chi2", VP), ("bad", VP), ("pose_state", VP), ("iters", C.c_int32 * 2),
                ("n_frames", C.c_int32), ("n_points", C.c_int32), ("n_obs", C.c_int32)]


OBS_DTYPE = np.dtype([("point", np.int32), ("frame", np.int32), ("u", np.float32), ("v", np.float32), ("inv_sigma", np.float64)])   # uh_ba_obs, 24 B


def _declare(L, sig):
    sig("uh_ba_create", I, VP, C.POINTER(VP))
    sig("uh_ba_destroy", None, VP)
    sig("uh_ba_set_problem", I, VP, C.POINTER(_Problem), C.POINTER(ParamSet))
    sig("uh_ba_optimize", I, VP, VP)
    sig("uh_ba_optimize_async", I, VP, VP)
    sig("uh_ba_wait", I, VP)
    sig("uh_ba_stop_flag", VP, VP)
    sig("uh_ba_get_results", I, VP, VP, VP, VP, VP, VP)
    sig("uh_ba_get_pose_state", I, VP, VP)
    sig("uh_ba_map_staging", I, VP, I, I, I, C.POINTER(_Staging))
    sig("uh_ba_set_problem_staged", I, VP, I, I, I, C.POINTER(ParamSet))
    sig("uh_ba_results_view_get", I, VP, C.POINTER(_ResultsView))
    sig("uh_ba_solve_async", I, VP, C.POINTER(_Problem), I, I, I, C.POINTER(ParamSet), VP)
    sig("uh_ba_form", I, VP, C.POINTER(C.c_int))
    sig("uh_ba_want_chi2", I, VP, I)
    sig("uh_ba_set_problem_stereo", I, VP, C.POINTER(_Problem), C.POINTER(_Stereo), C.POINTER(ParamSet))
    sig("uh_ba_map_staging_stereo", I, VP, I, I, I, C.POINTER(_StagingStereo))
    sig("uh_ba_set_problem_staged_stereo", I, VP, I, I, I, C.POINTER(ParamSet), C.c_double, C.c_double)
    sig("uh_ba_set_problem_markers", I, VP, C.POINTER(_Problem), C.POINTER(_Stereo), C.POINTER(_Markers), C.POINTER(ParamSet))
    sig("uh_ba_get_marker_results", I, VP, VP, VP, VP)
    sig("uh_ba_debug_solve", I, VP, I, I, VP, VP, VP, VP, C.POINTER(C.c_int))


# uh_ba_debug_solve: free keyframes a form holds, and whether it keeps D on the diagonal
SOLVE_FORMS = {1: (1, 10, False), 2: (11, 16, False), 3: (1, 10, False), 4: (11, 21, False), 5: (1, 32, True), 6: (1, 64, True), 7: (1, 341, True)}


def split_factor(LD, keeps_d: bool, blocked: bool = False):
    """(L, D or None, z) from the (n + 1) x (n + 1) matrix a solve form leaves: L unit lower with everything a form documents as garbage (on
    and above the diagonal, column n) masked out, D where the form keeps it, z = D^-1 L^-1 b from row n.  The blocked forms substitute in
    row n itself, panel by panel from the last one: only the last 64-column panel's part of it is still z, the rest is NaN here."""
    n = LD.shape[0] - 1
    L = np.tril(LD[:n, :n], -1) + np.eye(n)
    z = LD[n, :n].copy()
    if blocked:
        z[:((n - 1) // 64) * 64] = np.nan
    return L, (np.diag(LD)[:n].copy() if keeps_d else None), z


_lib._EXTRA_DECLS.append(_declare)


class GlobalOptimizer:
    def __init__(self, ctx: _lib.Context):
        self.ctx = ctx
        self._h = VP()
        check(lib().uh_ba_create(ctx.handle, C.byref(self._h)))
        self._dims = None
        self._bad = None

    @staticmethod
    def create(ctx: _lib.Context, type: str = "hip") -> "GlobalOptimizer":
        if type not in ("", "hip"):                       # globaloptimizer.cpp:27-33: unknown type throws
            raise RuntimeError("GlobalOptimizer::create: invalid optimizer type " + type)
        return GlobalOptimizer(ctx)

    def getName(self) -> str:
        return "hip"

    def _problem_struct(self, problem: dict):
        a = {k: np.ascontiguousarray(problem[k]) for k in ("poses", "fixed", "intr", "points", "obs_pt", "obs_kf", "obs_uv", "obs_w")}
        assert a["poses"].dtype == np.float32 and a["intr"].dtype == np.float32 and a["points"].dtype == np.float32
        assert a["obs_pt"].dtype == np.int32 and a["obs_kf"].dtype == np.int32 and a["obs_uv"].dtype == np.float32
        assert a["obs_w"].dtype == np.float64 and a["fixed"].dtype == np.uint8
        K, P, E = len(a["fixed"]), len(a["points"]), len(a["obs_pt"])
        pr = _Problem(K, P, E, np_ptr(a["poses"]), np_ptr(a["fixed"]), np_ptr(a["intr"]), np_ptr(a["points"]), np_ptr(a["obs_pt"]),
                      np_ptr(a["obs_kf"]), np_ptr(a["obs_uv"]), np_ptr(a["obs_w"]))
        return pr, a, (K, P, E)

    @staticmethod
    def _markers_struct(markers: dict):
        m = dict(pose_g2m=np.ascontiguousarray(markers["pose_g2m"], np.float32).reshape(-1, 16), size=np.ascontiguousarray(markers["size"], np.float32),
                 edge_marker=np.ascontiguousarray(markers["edge_marker"], np.int32), edge_frame=np.ascontiguousarray(markers["edge_frame"], np.int32),
                 und_corners=np.ascontiguousarray(markers["und_corners"], np.float32).reshape(-1, 8),
                 edge_weight=np.ascontiguousarray(markers["edge_weight"], np.float64))
        M, EM = len(m["size"]), len(m["edge_marker"])
        assert len(m["pose_g2m"]) == M and len(m["edge_frame"]) == EM and len(m["und_corners"]) == EM and len(m["edge_weight"]) == EM
        return _Markers(M, np_ptr(m["pose_g2m"]), np_ptr(m["size"]), EM, np_ptr(m["edge_marker"]), np_ptr(m["edge_frame"]), np_ptr(m["und_corners"]),
                        np_ptr(m["edge_weight"])), m, (M, EM)

    def setParams(self, problem, params: ParamSet | None = None, stereo=None, markers=None):
        """stereo: None (monocular edges only, uh_ba_set_problem), True (the problem dict's "obs_depth" [E] f32 and "frame_bl" [K] f32:
        an observation with depth > 0 is a three-row stereo / RGB-D edge) or a dict(huber_delta_3d=, chi2_threshold_3d=) with that meaning.
        markers: None, or a dict(pose_g2m [M,16] f32, size [M] f32, edge_marker [EM] i32, edge_frame [EM] i32, und_corners [EM,8] f32,
        edge_weight [EM] f64): squared planar markers with free poses (uh_ba_set_problem_markers); getMarkerResults() returns them."""
        pr, a, dims = problem if isinstance(problem, tuple) else self._problem_struct(problem)
        pp = C.byref(params) if params is not None else None
        sx = None
        if not (stereo is None or stereo is False):
            opts = stereo if isinstance(stereo, dict) else {}
            depth = np.ascontiguousarray(problem["obs_depth"], np.float32)
            bl = np.ascontiguousarray(problem["frame_bl"], np.float32)
            assert len(depth) == dims[2] and len(bl) == dims[0]
            sx = _Stereo(np_ptr(depth), np_ptr(bl), float(opts.get("huber_delta_3d", 0.0)), float(opts.get("chi2_threshold_3d", 0.0)))
        self._mdims = None
        if markers is not None:
            mk, keep, mdims = self._markers_struct(markers)
            check(lib().uh_ba_set_problem_markers(self._h, C.byref(pr), C.byref(sx) if sx is not None else None, C.byref(mk), pp))
            self._mdims = mdims if mdims[1] > 0 else None
        elif sx is None:
            check(lib().uh_ba_set_problem(self._h, C.byref(pr), pp))
        else:
            check(lib().uh_ba_set_problem_stereo(self._h, C.byref(pr), C.byref(sx), pp))
        self._dims = dims
        self._obs = (a["obs_pt"], a["obs_kf"])
        self._bad = None

    # ---- the staged form: the flattened problem is written straight into the optimiser's pinned staging block
    def mapStaging(self, K: int, P: int, max_obs: int) -> dict:
        """numpy views of the staging block (uh_ba_map_staging): poses [K,16] f32, fixed [K] u8, intr [K,4] f32, points [P,3] f32,
        obs [max_obs] records (OBS_DTYPE).  Valid until the next mapStaging / setParams on this object."""
        st = _Staging()
        check(lib().uh_ba_map_staging(self._h, K, P, max_obs, C.byref(st)))

        def view(ptr, dtype, shape):
            n = int(np.prod(shape)) * np.dtype(dtype).itemsize
            return np.frombuffer((C.c_char * n).from_address(ptr), dtype=dtype).reshape(shape)

        return dict(poses=view(st.poses_f2g, np.float32, (K, 16)), fixed=view(st.fixed, np.uint8, (K,)), intr=view(st.intr, np.float32, (K, 4)),
                    points=view(st.points, np.float32, (P, 3)), obs=view(st.obs, OBS_DTYPE, (max_obs,)))

    def fillStaging(self, problem: dict) -> tuple:
        """Copies a flattened problem dict into the staging block (what flatten_for_ba does in C++ while it walks the map)."""
        K, P, E = len(problem["fixed"]), len(problem["points"]), len(problem["obs_pt"])
        m = self.mapStaging(K, P, E)
        m["poses"][:] = problem["poses"].reshape(K, 16); m["fixed"][:] = problem["fixed"]; m["intr"][:] = problem["intr"]
        m["points"][:] = problem["points"]
        o = m["obs"]
        o["point"] = problem["obs_pt"]; o["frame"] = problem["obs_kf"]; o["u"] = problem["obs_uv"][:, 0]; o["v"] = problem["obs_uv"][:, 1]
        o["inv_sigma"] = problem["obs_w"]
        self._obs = (np.array(problem["obs_pt"], np.int32), np.array(problem["obs_kf"], np.int32))
        return K, P, E

    def fillStagingStereo(self, problem: dict) -> tuple:
        """fillStaging through uh_ba_map_staging_stereo: also the per-observation depth and the per-frame baseline."""
        K, P, E = len(problem["fixed"]), len(problem["points"]), len(problem["obs_pt"])
        st = _StagingStereo()
        check(lib().uh_ba_map_staging_stereo(self._h, K, P, E, C.byref(st)))

        def view(ptr, dtype, shape):
            n = int(np.prod(shape)) * np.dtype(dtype).itemsize
            return np.frombuffer((C.c_char * max(n, 1)).from_address(ptr), dtype=dtype, count=int(np.prod(shape))).reshape(shape)

        view(st.poses_f2g, np.float32, (K, 16))[:] = problem["poses"].reshape(K, 16)
        view(st.fixed, np.uint8, (K,))[:] = problem["fixed"]
        view(st.intr, np.float32, (K, 4))[:] = problem["intr"]
        view(st.points, np.float32, (P, 3))[:] = problem["points"]
        o = view(st.obs, OBS_DTYPE, (E,))
        o["point"] = problem["obs_pt"]; o["frame"] = problem["obs_kf"]; o["u"] = problem["obs_uv"][:, 0]; o["v"] = problem["obs_uv"][:, 1]
        o["inv_sigma"] = problem["obs_w"]
        view(st.obs_depth, np.float32, (E,))[:] = problem["obs_depth"]
        view(st.frame_bl, np.float32, (K,))[:] = problem["frame_bl"]
        self._obs = (np.array(problem["obs_pt"], np.int32), np.array(problem["obs_kf"], np.int32))
        return K, P, E

    def setParamsStagedStereo(self, K: int, P: int, E: int, params: ParamSet | None = None, huber_delta_3d=0.0, chi2_threshold_3d=0.0):
        check(lib().uh_ba_set_problem_staged_stereo(self._h, K, P, E, C.byref(params) if params is not None else None,
                                                    float(huber_delta_3d), float(chi2_threshold_3d)))
        self._dims = (K, P, E)
        self._bad = None

    def setParamsStaged(self, K: int, P: int, E: int, params: ParamSet | None = None):
        check(lib().uh_ba_set_problem_staged(self._h, K, P, E, C.byref(params) if params is not None else None))
        self._dims = (K, P, E)
        self._bad = None

    def solve_async(self, problem: dict | None, params: ParamSet | None = None, dims=None, stop_asap: np.ndarray | None = None):
        """setParams + optimize on the object's worker thread (the reference's mapper thread runs exactly these two calls back to back,
        mapmanager.cpp:11388-11405); `problem=None`: the staging block with `dims = (K, P, E)`.  wait() returns when both are done."""
        self._stop_keep = stop_asap
        self._params_keep = params
        if problem is not None:
            pr, a, dims = problem if isinstance(problem, tuple) else self._problem_struct(problem)   # (a tuple: prepareProblem()'s result)
            self._keep = (pr, a)
            self._obs = (a["obs_pt"], a["obs_kf"])
            check(lib().uh_ba_solve_async(self._h, C.byref(pr), 0, 0, 0, C.byref(params) if params is not None else None,
                                          np_ptr(stop_asap) if stop_asap is not None else None))
        else:
            check(lib().uh_ba_solve_async(self._h, None, dims[0], dims[1], dims[2], C.byref(params) if params is not None else None,
                                          np_ptr(stop_asap) if stop_asap is not None else None))
        self._dims = tuple(dims)
        self._bad = None

    def prepareProblem(self, problem: dict):
        """The ctypes view of a flattened problem, built once (solve_async / setParams accept it in place of the dict)."""
        return self._problem_struct(problem)

    def wantChi2(self, on: bool):
        """The per-observation chi2 is an extra of this ABI; switching it off (before setParams) shortens the kernel's result hand-over."""
        check(lib().uh_ba_want_chi2(self._h, int(on)))
        return self

    def form(self) -> str:
        """'persist<NF>' (one persistent launch, NF lanes per landmark), 'chain' (launch chain) or 'wide' (global BA)."""
        lanes = C.c_int(0)
        f = lib().uh_ba_form(self._h, C.byref(lanes))
        if f < 0:
            check(f)
        return {0: "chain", 1: f"persist{lanes.value}", 2: "wide"}[f]

    def resultsView(self) -> dict:
        """getResults in place (uh_ba_results_view_get): numpy views of the pinned result block, valid until the next setParams."""
        v = _ResultsView()
        check(lib().uh_ba_results_view_get(self._h, C.byref(v)))
        K, P, E = v.n_frames, v.n_points, v.n_obs

        def view(ptr, dtype, shape):
            n = int(np.prod(shape)) * np.dtype(dtype).itemsize
            return np.frombuffer((C.c_char * max(n, 1)).from_address(ptr), dtype=dtype, count=int(np.prod(shape))).reshape(shape)

        return dict(poses=view(v.poses, np.float32, (K, 16)), points=view(v.points, np.float32, (P, 3)), chi2=view(v.chi2, np.float64, (E,)),
                    bad=view(v.bad, np.uint8, (E,)), state=view(v.pose_state, np.float64, (K, 7)), iters=np.array(list(v.iters), np.int32))

    def debug_solve(self, form: int, S, b) -> dict:
        """Test hook (uh_ba_debug_solve): S x = b through one production solve form (SOLVE_FORMS), S (n, n) with n = 6 nfree, only its lower
        triangle read.  dict(x, failed, L, D (None where the form does not keep it), z, LD (the raw (n + 1, n + 1) matrix))."""
        S = np.ascontiguousarray(S, np.float64)
        b = np.ascontiguousarray(b, np.float64)
        n = len(b)
        if S.shape != (n, n) or n % 6:
            raise ValueError("debug_solve: S must be (n, n) and b (n,) with n a multiple of 6")
        x = np.zeros(n)
        LD = np.zeros((n + 1, n + 1))
        failed = C.c_int(-1)
        check(lib().uh_ba_debug_solve(self._h, int(form), n // 6, np_ptr(S), np_ptr(b), np_ptr(x), np_ptr(LD), C.byref(failed)))
        L, D, z = split_factor(LD, SOLVE_FORMS[form][2], blocked=form == 7)
        return dict(x=x, failed=int(failed.value), L=L, D=D, z=z, LD=LD)

    def optimize(self, stop_asap: np.ndarray | None = None):
        check(lib().uh_ba_optimize(self._h, np_ptr(stop_asap) if stop_asap is not None else None))

    def optimize_async(self, stop_asap: np.ndarray | None = None):
        """Starts optimize() on the object's worker thread (the reference's mapper thread); wait() returns when it is done."""
        self._stop_keep = stop_asap
        check(lib().uh_ba_optimize_async(self._h, np_ptr(stop_asap) if stop_asap is not None else None))

    def wait(self):
        check(lib().uh_ba_wait(self._h))

    def getResults(self):
        K, P, E = self._dims
        out = dict(poses=np.zeros((K, 16), np.float32), points=np.zeros((P, 3), np.float32), chi2=np.zeros(E, np.float64),
                   bad=np.zeros(E, np.uint8), iters=np.zeros(2, np.int32), state=np.zeros((K, 7), np.float64))
        check(lib().uh_ba_get_results(self._h, np_ptr(out["poses"]), np_ptr(out["points"]), np_ptr(out["chi2"]), np_ptr(out["bad"]),
                                      np_ptr(out["iters"])))
        check(lib().uh_ba_get_pose_state(self._h, np_ptr(out["state"])))
        self._bad_flags = out["bad"]
        self._bad = None
        return out

    def getMarkerResults(self):
        """After optimize() on a problem set with markers: dict(poses [M,16] f32 — Marker::pose_g2m as getResults writes it back —,
        state [M,7] f64 (qx qy qz qw tx ty tz), chi2 [EM] f64 of the marker edges at the final estimate)."""
        if getattr(self, "_mdims", None) is None:
            raise RuntimeError("GlobalOptimizer::getMarkerResults: the current problem has no markers")
        M, EM = self._mdims
        out = dict(poses=np.zeros((M, 16), np.float32), state=np.zeros((M, 7), np.float64), chi2=np.zeros(EM, np.float64))
        check(lib().uh_ba_get_marker_results(self._h, np_ptr(out["poses"]), np_ptr(out["state"]), np_ptr(out["chi2"])))
        return out

    def getBadAssociations(self):
        """vector<pair<point id, frame id>> (globaloptimizer.h:60)."""
        if self._bad is None and getattr(self, "_bad_flags", None) is not None:
            sel = np.flatnonzero(self._bad_flags)
            self._bad = [(int(p), int(f)) for p, f in zip(self._obs[0][sel], self._obs[1][sel])]
        return self._bad or []

    def close(self):
        if self._h:
            lib().uh_ba_destroy(self._h)
            self._h = VP()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
