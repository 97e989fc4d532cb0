"""Host-side mirror of ucoslam::PnPSolver::solvePnp (monocular, stereo and RGB-D matches) on top of the C ABI.

Reference: src/optimization/pnpsolver.h:30-38 / pnpsolver.cpp:116-409: `solvePnp(frame, map, matches, pose)` refines `pose`
in place, marks outlier matches (DMatch::imgIdx = -1, inliers = 1) and returns the number of inliers.
Here the frame/map lookups are already done: the caller passes, per match, the map point, the undistorted keypoint,
1/scaleFactor[octave] and the stability weight (1, or 0.5 for MapPoint::isStable() == false).  Stereo / RGB-D frames also pass
Frame::getDepth(queryIdx) per match (<= 0: monocular match) and imageParams.bl (pnpsolver.cpp:205-276).  A host that runs with markers
passes the frame's selected markers (pnpsolver.cpp:281-299) as three arrays: Marker::pose_g2m, Marker::size and
MarkerObservation::und_corners (:301-347).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import I, VP, check, lib, np_ptr


MAX_MARKERS = 32   # UH_PNP_MAX_MARKERS


class _Markers(C.Structure):   # uh_pnp_markers
    _fields_ = [("n", C.c_int32), ("pose_g2m", VP), ("size", VP), ("und_corners", VP)]


def pack_markers(markers):
    """dict(pose_g2m [m, 16] or [m, 4, 4], size [m], und_corners [m, 8] or [m, 4, 2]) -> (uh_pnp_markers, the arrays it points into)."""
    g2m = np.ascontiguousarray(markers["pose_g2m"], np.float32).reshape(-1, 16)
    size = np.ascontiguousarray(markers["size"], np.float32).reshape(-1)
    corners = np.ascontiguousarray(markers["und_corners"], np.float32).reshape(-1, 8)
    if not (len(g2m) == len(size) == len(corners)):
        raise ValueError(f"markers: {len(g2m)} poses, {len(size)} sizes, {len(corners)} corner sets")
    keep = (g2m, size, corners)
    return _Markers(len(size), np_ptr(g2m), np_ptr(size), np_ptr(corners)), keep


def _declare(L, sig):
    sig("uh_pnp_create", I, VP, C.POINTER(VP))
    sig("uh_pnp_destroy", None, VP)
    sig("uh_pnp_solve", I, VP, VP, VP, I, VP, VP, VP, VP, VP, VP, VP, VP)
    sig("uh_pnp_solve_dev", I, VP, VP, VP, I, VP, VP, VP, VP, VP, VP, VP, VP, VP)
    sig("uh_pnp_solve_stereo", I, VP, VP, VP, I, VP, VP, VP, VP, VP, C.c_float, VP, VP, VP, VP)
    sig("uh_pnp_solve_stereo_dev", I, VP, VP, VP, I, VP, VP, VP, VP, VP, C.c_float, VP, VP, VP, VP, VP)
    sig("uh_pnp_solve_markers", I, VP, VP, VP, I, VP, VP, VP, VP, VP, C.c_float, C.POINTER(_Markers), VP, VP, VP, VP)
    sig("uh_pnp_solve_markers_dev", I, VP, VP, VP, I, VP, VP, VP, VP, VP, C.c_float, C.POINTER(_Markers), VP, VP, VP, VP, VP)
    sig("uh_pnp_debug_clocks", I, VP, I, VP)


_lib._EXTRA_DECLS.append(_declare)


class PnPSolver:
    def __init__(self, ctx: _lib.Context):
        self.ctx = ctx
        self._h = VP()
        check(lib().uh_pnp_create(ctx.handle, C.byref(self._h)))

    def solvePnp(self, pose_f2g, intr, p3d, kp, inv_sigma, weight, depth=None, bl=0.0, markers=None):
        """Returns dict(pose [16] float32, bad [n] uint8, iters [4], state [7] fp64, ngood).  depth: None (monocular) or [n] float32
        Frame::getDepth per match, with bl = imageParams.bl (> 0 when any depth is > 0).  markers: None, or dict(pose_g2m [m, 16], size [m],
        und_corners [m, 8]) of the frame's selected markers (at most MAX_MARKERS); with markers n = 0 matches is a valid solve."""
        a = [np.ascontiguousarray(x, np.float32) for x in (pose_f2g, intr, p3d, kp, inv_sigma, weight)]
        n = len(a[4])
        out = dict(pose=np.zeros(16, np.float32), bad=np.zeros(max(n, 1), np.uint8), iters=np.zeros(4, np.int32), state=np.zeros(7, np.float64))
        mk, keep = pack_markers(markers) if markers is not None else (None, None)
        d = None
        if depth is not None:
            d = np.ascontiguousarray(depth, np.float32)
            if d.shape != (n,):
                raise ValueError(f"depth: expected {n} values, got shape {d.shape}")
        common = (self._h, np_ptr(a[0]), np_ptr(a[1]), n, np_ptr(a[2]), np_ptr(a[3]), np_ptr(a[4]), np_ptr(a[5]))
        res = (np_ptr(out["pose"]), np_ptr(out["bad"]), np_ptr(out["iters"]), np_ptr(out["state"]))
        if mk is not None:
            rc = lib().uh_pnp_solve_markers(*common, None if d is None else np_ptr(d), float(bl), C.byref(mk), *res)
            del keep
        elif d is None:
            rc = lib().uh_pnp_solve(*common, *res)
        else:
            rc = lib().uh_pnp_solve_stereo(*common, np_ptr(d), float(bl), *res)
        if rc < 0:
            check(rc)
        out["ngood"] = rc
        out["bad"] = out["bad"][:n]
        return out

    def debug_clocks(self, on=True):
        """Shader-clock stamps of the last solve (measurement hook): [entry, staged, rounds done, posted, passes, ...]."""
        out = np.zeros(512, np.int64)
        check(lib().uh_pnp_debug_clocks(self._h, int(on), np_ptr(out)))
        return out

    def close(self):
        if self._h:
            lib().uh_pnp_destroy(self._h)
            self._h = VP()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
