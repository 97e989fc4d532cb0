"""Host-side mirror of MapInitializer's two-view initialise (src/utils/mapinitializer.cpp:152-201) on top of the C ABI.  See
include/ucoslam_hip.h for the contract, csrc/mapinit.hip for the kernels, csrc/mapinit_math.hpp for the arithmetic."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import I, VP, check, lib, np_ptr

MAX_ITERS, MAX_MATCHES = 1024, 16384
NONE, HOMOGRAPHY, FUNDAMENTAL = 0, 1, 2
NOT_INLIER, REJECTED, COUNTED_LOW_PARALLAX, COUNTED_GOOD, NON_FINITE = 0, 1, 2, 3, 4


class _Args(C.Structure):   # uh_mapinit_args
    _fields_ = [("intr4", VP), ("kp1", VP), ("n_kp1", C.c_int32), ("kp2", VP), ("n_kp2", C.c_int32), ("matches", VP), ("n_matches", C.c_int32),
                ("sigma", C.c_float), ("iterations", C.c_int32), ("min_matches", C.c_int32), ("min_parallax", C.c_float),
                ("min_triangulated", C.c_int32), ("min_distance", C.c_float), ("samples", VP)]


class _Result(C.Structure):   # uh_mapinit_result
    _fields_ = [("ok", C.c_int32), ("model", C.c_int32), ("winner", C.c_int32), ("best_h", C.c_int32), ("best_f", C.c_int32),
                ("score_h", C.c_float), ("score_f", C.c_float), ("rh", C.c_float), ("n_candidates", C.c_int32), ("n_inliers", C.c_int32),
                ("n_good", C.c_int32 * 8), ("parallax", C.c_float * 8), ("R", C.c_float * 9), ("t", C.c_float * 3), ("pose", C.c_float * 16),
                ("n_out", C.c_int32), ("matches_out", VP), ("points_out", VP), ("triangulated", VP), ("p3d", VP), ("state", VP),
                ("index_out", VP), ("cap_matches", C.c_int32)]


def _declare(L, sig):
    sig("uh_mapinit_create", I, VP, C.POINTER(VP))
    sig("uh_mapinit_destroy", None, VP)
    sig("uh_mapinit_run", I, VP, C.POINTER(_Args), C.POINTER(_Result))
    sig("uh_mapinit_run_host", I, C.POINTER(_Args), C.POINTER(_Result))
    sig("uh_mapinit_samples", I, C.c_int32, C.c_int32, VP)
    sig("uh_mapinit_debug_hypothesis", I, VP, C.POINTER(_Args), C.c_int32, C.c_int32, VP, VP, C.POINTER(C.c_float), VP)
    sig("uh_mapinit_debug_reconstruct", I, VP, C.POINTER(_Args), C.c_int32, VP, VP, C.POINTER(_Result))


_lib._EXTRA_DECLS.append(_declare)


def mapinit_samples(n: int, iterations: int) -> np.ndarray:
    """uh_mapinit_samples: (iterations, 8) int32, the reference's draw.  Calls libc's srand(0) as the reference does.  Host only."""
    out = np.zeros((max(int(iterations), 0), 8), np.int32)
    check(lib().uh_mapinit_samples(int(n), int(iterations), np_ptr(out)))
    return out


def _pack(intr4, kp1, kp2, matches, sigma, iterations, min_matches, min_parallax, min_triangulated, min_distance, samples, n_matches=None):
    keep = {}
    keep["intr"] = np.ascontiguousarray(intr4, np.float32).reshape(4)
    keep["kp1"] = np.ascontiguousarray(kp1, np.float32).reshape(-1, 2)
    keep["kp2"] = np.ascontiguousarray(kp2, np.float32).reshape(-1, 2)
    keep["m"] = np.ascontiguousarray(matches, np.int32).reshape(-1, 2)
    a = _Args()
    a.intr4, a.kp1, a.n_kp1, a.kp2, a.n_kp2 = np_ptr(keep["intr"]), np_ptr(keep["kp1"]), len(keep["kp1"]), np_ptr(keep["kp2"]), len(keep["kp2"])
    a.matches, a.n_matches = np_ptr(keep["m"]), len(keep["m"]) if n_matches is None else int(n_matches)
    a.sigma, a.iterations, a.min_matches, a.min_parallax = float(sigma), int(iterations), int(min_matches), float(min_parallax)
    a.min_triangulated, a.min_distance = int(min_triangulated), float(min_distance)
    if samples is not None:
        keep["s"] = np.ascontiguousarray(samples, np.int32).reshape(-1, 8)
        a.samples = np_ptr(keep["s"])
    else:
        a.samples = None
    n, nk = max(len(keep["m"]), 1), max(len(keep["kp1"]), 1)
    keep["mo"], keep["po"] = np.zeros((n, 2), np.int32), np.zeros((n, 3), np.float32)
    keep["tri"], keep["p3d"], keep["st"] = np.zeros(nk, np.uint8), np.zeros((nk, 3), np.float32), np.zeros(n, np.uint8)
    keep["at"] = np.zeros(n, np.int32)
    r = _Result()
    r.matches_out, r.points_out, r.triangulated, r.p3d, r.state, r.index_out = (np_ptr(keep[k]) for k in ("mo", "po", "tri", "p3d", "st", "at"))
    r.cap_matches = len(keep["m"])
    return a, r, keep


def _unpack(r, keep):
    n, nk = r.n_out, len(keep["kp1"])
    return dict(ok=int(r.ok), model=int(r.model), winner=int(r.winner), best_h=int(r.best_h), best_f=int(r.best_f),
                score_h=np.float32(r.score_h), score_f=np.float32(r.score_f), rh=np.float32(r.rh), n_candidates=int(r.n_candidates),
                n_inliers=int(r.n_inliers), n_good=np.array(r.n_good[:], np.int32), parallax=np.array(r.parallax[:], np.float32),
                R=np.array(r.R[:], np.float32).reshape(3, 3), t=np.array(r.t[:], np.float32), pose=np.array(r.pose[:], np.float32).reshape(4, 4),
                matches=keep["mo"][:n].copy(), points=keep["po"][:n].copy(), triangulated=keep["tri"][:nk].astype(bool),
                p3d=keep["p3d"][:nk].copy(), state=keep["st"][:len(keep["m"])].copy(), index=keep["at"][:n].copy())


_DEFAULTS = dict(sigma=1.0, iterations=200, min_matches=50, min_parallax=1.0, min_triangulated=50, min_distance=0.1, samples=None)


def initialize_host(intr4, kp1, kp2, matches, **kw):
    """uh_mapinit_run_host: the whole stage on the calling core.  Returns the dict MapInit.initialize returns."""
    p = dict(_DEFAULTS, **kw)
    a, r, keep = _pack(intr4, kp1, kp2, matches, **p)
    check(lib().uh_mapinit_run_host(C.byref(a), C.byref(r)))
    return _unpack(r, keep)


def _reconstruct(handle, intr4, kp1, kp2, matches, model, M, mask, **kw):
    a, r, keep = _pack(intr4, kp1, kp2, matches, **dict(_DEFAULTS, **kw))
    n = len(keep["m"])
    bits = np.zeros(((n + 63) // 64 or 1) * 64, np.uint8)
    bits[:n] = np.asarray(mask, bool)[:n]
    words = np.packbits(bits, bitorder="little").view(np.uint64)
    Mf = np.ascontiguousarray(M, np.float32).reshape(9)
    check(lib().uh_mapinit_debug_reconstruct(handle, C.byref(a), int(model), np_ptr(Mf), np_ptr(words), C.byref(r)))
    return _unpack(r, keep)


def debug_reconstruct_host(intr4, kp1, kp2, matches, model, M, mask, **kw):
    """Test hook, host form: the reconstruction alone on a planted float model matrix M (3, 3) and inlier mask (n) bool."""
    return _reconstruct(None, intr4, kp1, kp2, matches, model, M, mask, **kw)


class MapInit:
    """uh_mapinit: the two-view initialiser on the device."""

    def __init__(self, ctx):
        self._h = VP()
        self._ctx = ctx
        check(lib().uh_mapinit_create(ctx.handle, C.byref(self._h)))

    def prepare(self, intr4, kp1, kp2, matches, **kw):
        """The C structures of a call, built once: a zero-argument function that runs uh_mapinit_run on them (what scripts/time_mapinit.py
        times), and what initialize() reads the result from."""
        p = dict(_DEFAULTS, **kw)
        a, r, keep = _pack(intr4, kp1, kp2, matches, **p)
        fn, h, pa, pr = lib().uh_mapinit_run, self._h, C.byref(a), C.byref(r)
        return (lambda: fn(h, pa, pr)), a, r, keep

    def initialize(self, intr4, kp1, kp2, matches, **kw):
        """kp1 (n1, 2) und_kpts of the reference frame, kp2 (n2, 2) of the second, matches (n, 2) int32 (trainIdx -> kp1, queryIdx -> kp2).
        Returns dict(ok, model, winner, best_h, best_f, score_h, score_f, rh, n_candidates, n_inliers, n_good (8), parallax (8), R, t, pose
        (4, 4), matches (n_out, 2), points (n_out, 3), triangulated (n1) bool, p3d (n1, 3), state (n) uint8)."""
        call, _a, r, keep = self.prepare(intr4, kp1, kp2, matches, **kw)
        check(call())
        return _unpack(r, keep)

    def debug_hypothesis(self, intr4, kp1, kp2, matches, model, it, **kw):
        """Test hook: dict(M (3, 3) float64, Mf (3, 3) float32, score, mask (n) bool) of one hypothesis, from the device."""
        p = dict(_DEFAULTS, **kw)
        a, _r, keep = _pack(intr4, kp1, kp2, matches, **p)
        n = len(keep["m"])
        M, Mf, sc, words = np.zeros(9), np.zeros(9, np.float32), C.c_float(0), np.zeros(max((n + 63) // 64, 1), np.uint64)
        check(lib().uh_mapinit_debug_hypothesis(self._h, C.byref(a), int(model), int(it), np_ptr(M), np_ptr(Mf), C.byref(sc), np_ptr(words)))
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)
        return dict(M=M.reshape(3, 3), Mf=Mf.reshape(3, 3), score=np.float32(sc.value), mask=bits)

    def debug_reconstruct(self, intr4, kp1, kp2, matches, model, M, mask, **kw):
        """Test hook: the second launch alone on a planted float model matrix M (3, 3) and inlier mask (n) bool."""
        return _reconstruct(self._h, intr4, kp1, kp2, matches, model, M, mask, **kw)

    def close(self):
        if self._h:
            lib().uh_mapinit_destroy(self._h)
            self._h = VP()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
