"""Host-side mirror of ucoslam::PnPSolver::solvePnPRansac (src/optimization/pnpsolver.cpp:36-114) on top of the C ABI: the relocalisation
RANSAC, batched over the candidate keyframes of one lost frame.  See include/ucoslam_hip.h for the contract, csrc/pnp_ransac.hip for
the kernels, csrc/p3p_math.hpp for the arithmetic."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import I, VP, check, lib, np_ptr

MAX_PROBLEMS, MAX_ITERS, MAX_MATCHES = 64, 1024, 16384


class _Problem(C.Structure):   # uh_ransac_problem
    _fields_ = [("n", C.c_int32), ("p3d", VP), ("normal", VP), ("kp", VP), ("iters", C.c_int32), ("samples", VP), ("rt6_in", VP)]


class _Result(C.Structure):   # uh_ransac_result
    _fields_ = [("ok", C.c_int32), ("n_inliers", C.c_int32), ("best_iter", C.c_int32), ("rt6", C.c_float * 6), ("pose", C.c_float * 16),
                ("inliers", VP), ("cap", C.c_int32), ("counts", VP)]


def _declare(L, sig):
    sig("uh_pnp_ransac", I, VP, VP, I, VP, VP)
    sig("uh_pnp_ransac_samples", I, I, I, VP)
    sig("uh_pnp_ransac_debug_form", I, VP, I)
    sig("uh_pnp_ransac_debug_roots", I, VP, I, VP, VP, VP)
    sig("uh_pnp_ransac_debug_hypothesis", I, VP, VP, C.POINTER(_Problem), I, C.POINTER(C.c_int32), VP, C.POINTER(C.c_int32), VP)


_lib._EXTRA_DECLS.append(_declare)


def ransac_samples(n: int, iters: int) -> np.ndarray:
    """uh_pnp_ransac_samples: (iters, 4) int32, drawn from libc rand() exactly as the reference's std::random_shuffle loop draws them
    (call libc's srand first for a chosen sequence).  Host only."""
    out = np.zeros((max(int(iters), 0), 4), np.int32)
    check(lib().uh_pnp_ransac_samples(int(n), int(iters), np_ptr(out)))
    return out


def _pack(pr, keep, n=None, iters=None):
    """One problem dict(p3d (n, 3), normal (n, 3), kp (n, 2), samples (iters, 4), rt6_in (6) [, n, iters]) -> uh_ransac_problem.  Arrays are
    converted, never range-checked here: that is the library's part (n / iters override the counts for its tests)."""
    def arr(x, dt, shape):
        a = np.ascontiguousarray(x, dt).reshape(shape)
        keep.append(a)
        return a

    p3d, nrm, kp = arr(pr["p3d"], np.float32, (-1, 3)), arr(pr["normal"], np.float32, (-1, 3)), arr(pr["kp"], np.float32, (-1, 2))
    smp, rt6 = arr(pr["samples"], np.int32, (-1, 4)), arr(pr["rt6_in"], np.float32, 6)
    q = _Problem()
    q.n = int(pr.get("n", len(p3d)) if n is None else n)
    q.iters = int(pr.get("iters", len(smp)) if iters is None else iters)
    q.p3d, q.normal, q.kp, q.samples, q.rt6_in = np_ptr(p3d), np_ptr(nrm), np_ptr(kp), np_ptr(smp), np_ptr(rt6)
    return q


class PnPRansac:
    """solvePnPRansac on a PnPSolver's uh_pnp object (or on one of its own when given a Context)."""

    def __init__(self, ctx_or_solver):
        self._own = None
        if hasattr(ctx_or_solver, "_h") and not isinstance(ctx_or_solver, _lib.Context):
            self._h = ctx_or_solver._h
            self._keep = ctx_or_solver
        else:
            self._own = VP()
            check(lib().uh_pnp_create(ctx_or_solver.handle, C.byref(self._own)))
            self._h = self._own
            self._keep = ctx_or_solver

    def prepare(self, intr4, problems, want_counts=True):
        """The C structures of a call, built once: returns a zero-argument function that runs uh_pnp_ransac on them (nothing but the C call:
        what scripts/time_pnp_ransac.py times) and everything solve() reads the results from."""
        intr = np.ascontiguousarray(intr4, np.float32).reshape(4)
        keep, m = [intr], len(problems)
        ps, rs = (_Problem * max(m, 1))(), (_Result * max(m, 1))()
        bufs = []
        for j, pr in enumerate(problems):
            ps[j] = _pack(pr, keep)
            inl = np.zeros(max(ps[j].n, 1), np.int32)
            cnt = np.zeros(max(ps[j].iters, 1), np.int32)
            bufs.append((inl, cnt))
            rs[j].inliers, rs[j].cap = np_ptr(inl), int(pr.get("cap", max(ps[j].n, 0)))
            rs[j].counts = np_ptr(cnt) if want_counts else None
        fn, h, pi, pp, pr_ = lib().uh_pnp_ransac, self._h, np_ptr(intr), C.cast(ps, VP), C.cast(rs, VP)
        return (lambda: fn(h, pi, m, pp, pr_)), ps, rs, bufs, keep

    def set_form(self, uniform_roots: bool):
        """Measurement hook (uh_pnp_ransac_debug_form): True = every lane takes all four roots; False (default) = one root per lane."""
        check(lib().uh_pnp_ransac_debug_form(self._h, int(bool(uniform_roots))))

    def solve(self, intr4, problems, want_counts=True):
        """problems: list of dict(p3d, normal, kp, samples, rt6_in) (one per candidate keyframe).  Returns a list of dict(ok, n_inliers,
        best_iter, rt6 (6), pose (4, 4), inliers (n_inliers) int32 ascending, counts (iters) int32 with -1 = skipped)."""
        m = len(problems)
        call, ps, rs, bufs, _keep = self.prepare(intr4, problems, want_counts)
        check(call())
        out = []
        for j in range(m):
            r = rs[j]
            out.append(dict(ok=int(r.ok), n_inliers=int(r.n_inliers), best_iter=int(r.best_iter), rt6=np.array(r.rt6[:], np.float32),
                            pose=np.array(r.pose[:], np.float32).reshape(4, 4), inliers=bufs[j][0][:r.n_inliers].copy(),
                            counts=bufs[j][1][:max(ps[j].iters, 0)].copy() if want_counts else None))
        return out

    def debug_hypothesis(self, intr4, problem, it):
        """Test hook: dict(n_solutions, Rt (n_solutions, 12) float64, chosen, rvec_tvec (6) float64) of one hypothesis, from the device."""
        intr = np.ascontiguousarray(intr4, np.float32).reshape(4)
        keep = []
        q = _pack(problem, keep)
        ns, ch = C.c_int32(0), C.c_int32(0)
        Rt, rv = np.zeros((4, 12)), np.zeros(6)
        check(lib().uh_pnp_ransac_debug_hypothesis(self._h, np_ptr(intr), C.byref(q), int(it), C.byref(ns), np_ptr(Rt), C.byref(ch), np_ptr(rv)))
        return dict(n_solutions=int(ns.value), Rt=Rt[:ns.value].copy(), chosen=int(ch.value), rvec_tvec=rv)

    def debug_roots(self, A):
        """Test hook: A (n, 5) float64, the coefficients A0..A4 of n quartics -> (roots (n, 4) float64 ascending with +inf for the absent
        ones, their number (n) int32), from the device's root finder."""
        A = np.ascontiguousarray(A, np.float64).reshape(-1, 5)
        r, k = np.zeros((len(A), 4)), np.zeros(len(A), np.int32)
        check(lib().uh_pnp_ransac_debug_roots(self._h, len(A), np_ptr(A), np_ptr(r), np_ptr(k)))
        return r, k

    def close(self):
        if self._own:
            lib().uh_pnp_destroy(self._own)
            self._own = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
