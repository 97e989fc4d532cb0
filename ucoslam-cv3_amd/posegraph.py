"""Loop-closure pose graph (uh_posegraph_*): loopClosurePathOptimizationg2o of the reference (graphoptsim3.cpp:74-168) — g2o's Levenberg
over Sim3 vertices and seven-row Sim3 edges on the essential graph — on the device.  See include/ucoslam_hip.h for the problem's
definition; csrc/posegraph.hip for the kernels."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import I, VP, check, lib, np_ptr

MAX_POSES = 2048
MAX_ITERS = 256


class _Problem(C.Structure):   # uh_posegraph_problem
    _fields_ = [("n_poses", C.c_int32), ("pose_f2g", VP), ("n_edges", C.c_int32), ("edge_i", VP), ("edge_j", VP), ("edge_weight", VP),
                ("idx_new", C.c_int32), ("idx_old", C.c_int32), ("expected_pose_new", VP), ("fix_scale", C.c_int32)]


class _Params(C.Structure):   # uh_posegraph_params
    _fields_ = [("max_iters", C.c_int32), ("lambda_init", C.c_double), ("fd_delta", C.c_float)]


class _Info(C.Structure):   # uh_posegraph_info
    _fields_ = [("iterations", C.c_int32), ("lambda_", C.c_double), ("chi2_before", C.c_double), ("chi2_after", C.c_double)]


def _declare(L, sig):
    sig("uh_posegraph_create", I, VP, C.POINTER(VP))
    sig("uh_posegraph_destroy", None, VP)
    sig("uh_posegraph_check_problem", I, C.POINTER(_Problem), C.POINTER(_Params))
    sig("uh_posegraph_optimize", I, VP, C.POINTER(_Problem), C.POINTER(_Params))
    sig("uh_posegraph_get_results", I, VP, VP, VP, C.POINTER(_Info), VP)
    sig("uh_posegraph_debug_linearisation", I, VP, VP, VP, VP, VP)
    sig("uh_posegraph_debug_solve", I, VP, I, VP, VP, VP, VP, C.POINTER(C.c_int))


_lib._EXTRA_DECLS.append(_declare)


def _pack(poses, edge_i, edge_j, edge_weight, idx_new, idx_old, expected_pose_new, fix_scale, n_poses=None):
    """(uh_posegraph_problem, the arrays it points into).  Arrays are converted, never range-checked here: that is the library's part."""
    keep = dict(poses=np.ascontiguousarray(poses, np.float32).reshape(-1, 16), edge_i=np.ascontiguousarray(edge_i, np.int32).ravel(),
                edge_j=np.ascontiguousarray(edge_j, np.int32).ravel(), expected=np.ascontiguousarray(expected_pose_new, np.float32).reshape(16),
                w=None if edge_weight is None or len(edge_weight) == 0 else np.ascontiguousarray(edge_weight, np.float32).ravel())
    if keep["edge_i"].shape != keep["edge_j"].shape or (keep["w"] is not None and keep["w"].shape != keep["edge_i"].shape):
        raise ValueError("edge_i, edge_j and edge_weight must have one entry per edge")
    pr = _Problem(len(keep["poses"]) if n_poses is None else n_poses, np_ptr(keep["poses"]), len(keep["edge_i"]), np_ptr(keep["edge_i"]),
                  np_ptr(keep["edge_j"]), np_ptr(keep["w"]) if keep["w"] is not None else None, int(idx_new), int(idx_old), np_ptr(keep["expected"]),
                  int(bool(fix_scale)))
    return pr, keep


def check_problem(poses, edge_i, edge_j, edge_weight, idx_new, idx_old, expected_pose_new, fix_scale, max_iters=0, lambda_init=0.0, fd_delta=0.0,
                  n_poses=None) -> int:
    """uh_posegraph_check_problem: the return code (UH_OK, UH_EINVAL, UH_ECAPACITY) of the argument checks; runs without a device."""
    pr, _keep = _pack(poses, edge_i, edge_j, edge_weight, idx_new, idx_old, expected_pose_new, fix_scale, n_poses)
    pa = _Params(int(max_iters), float(lambda_init), float(fd_delta))
    return int(lib().uh_posegraph_check_problem(C.byref(pr), C.byref(pa)))


class PoseGraph:
    def __init__(self, ctx: _lib.Context):
        self.ctx = ctx
        self._h = VP()
        check(lib().uh_posegraph_create(ctx.handle, C.byref(self._h)))
        self._n = self._E = self._max_iters = 0

    def optimize(self, poses, edge_i, edge_j, edge_weight, idx_new, idx_old, expected_pose_new, fix_scale, max_iters=0, lambda_init=0.0, fd_delta=0.0):
        """Returns dict(poses (n, 16) float32, state (n, 8) float64 = qx qy qz qw tx ty tz s, iterations, trials, lambda_, chi2_before,
        chi2_after).  0 for a parameter means the reference's value (20, 1e-16, 1e-9f)."""
        pr, keep = _pack(poses, edge_i, edge_j, edge_weight, idx_new, idx_old, expected_pose_new, fix_scale)
        pa = _Params(int(max_iters), float(lambda_init), float(fd_delta))
        check(lib().uh_posegraph_optimize(self._h, C.byref(pr), C.byref(pa)))
        self._n, self._E, self._max_iters = pr.n_poses, pr.n_edges, int(max_iters) or 20
        out_p = np.zeros((self._n, 16), np.float32)
        out_s = np.zeros((self._n, 8), np.float64)
        trials = np.zeros(self._max_iters, np.int32)
        info = _Info()
        check(lib().uh_posegraph_get_results(self._h, np_ptr(out_p), np_ptr(out_s), C.byref(info), np_ptr(trials)))
        return dict(poses=out_p, state=out_s, iterations=int(info.iterations), trials=trials[:info.iterations].copy(), lambda_=float(info.lambda_),
                    chi2_before=float(info.chi2_before), chi2_after=float(info.chi2_after))

    def debug_linearisation(self):
        """The first linearisation of the latest optimize: dict(err (E, 7), Ji (E, 7, 7), Jj (E, 7, 7), meas (E, 8))."""
        E = self._E
        o = dict(err=np.zeros((E, 7)), Ji=np.zeros((E, 7, 7)), Jj=np.zeros((E, 7, 7)), meas=np.zeros((E, 8)))
        check(lib().uh_posegraph_debug_linearisation(self._h, np_ptr(o["err"]), np_ptr(o["Ji"]), np_ptr(o["Jj"]), np_ptr(o["meas"])))
        return o

    def debug_solve(self, S, b) -> dict:
        """Test hook (uh_posegraph_debug_solve): S x = b through the optimiser's blocked LDL^T (csrc/dense_ldlt.hpp), S (n, n), only its lower
        triangle read.  dict(x, failed, L, D, z, LD (the raw (n + 1, n + 1) matrix)); x is unspecified where failed = 1."""
        from .ba import split_factor

        S = np.ascontiguousarray(S, np.float64)
        b = np.ascontiguousarray(b, np.float64)
        n = len(b)
        if S.shape != (n, n):
            raise ValueError("debug_solve: S must be (n, n) and b (n,)")
        x = np.zeros(n)
        LD = np.zeros((n + 1, n + 1))
        failed = C.c_int(-1)
        check(lib().uh_posegraph_debug_solve(self._h, n, np_ptr(S), np_ptr(b), np_ptr(x), np_ptr(LD), C.byref(failed)))
        L, D, z = split_factor(LD, True, blocked=True)
        return dict(x=x, failed=int(failed.value), L=L, D=D, z=z, LD=LD)

    def close(self):
        if self._h:
            lib().uh_posegraph_destroy(self._h)
            self._h = VP()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
