"""New map points (uh_newpoints_*): for one new keyframe and all its covisible neighbours, Triangulate (misc.cpp:923-1041), the
distance-ratio / octave-ratio check and the per-keypoint merge of MapManager (mapmanager.cpp:10087-10696) on the device; and
uh_fundamental_12, the F12 of the epipolar-gated matchers.  See include/ucoslam_hip.h for the contract, csrc/newpoints.hip for the
kernels."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import I, VP, check, lib, np_ptr
from .matcher import DMATCH_DTYPE

MAX_KPTS = 16384
MAX_PAIRS = 1024
MERGE_SMALLEST_OCTAVE, MERGE_AS_COMPILED = 0, 1
STATUS_NAMES = ("accepted", "parallax", "w == 0", "not finite", "depth in camera 1", "depth in camera 2", "chi2 in image 1",
                "chi2 in image 2", "zero distance", "scale ratio")


class _Pair(C.Structure):   # uh_newpoints_pair
    _fields_ = [("RT", C.c_float * 16), ("intr4", C.c_float * 4), ("cam_center", C.c_float * 3), ("n_levels", C.c_int32),
                ("scale_factors", VP), ("n_kpts", C.c_int32), ("pt", VP), ("octave", VP), ("n_matches", C.c_int32), ("matches", VP)]


class _Args(C.Structure):   # uh_newpoints_args
    _fields_ = [("intr4", C.c_float * 4), ("pose_g2f", C.c_float * 16), ("cam_center", C.c_float * 3), ("n_levels", C.c_int32),
                ("scale_factors", VP), ("n_kpts", C.c_int32), ("pt", VP), ("octave", VP), ("n_pairs", C.c_int32), ("pairs", VP),
                ("max_chi2", C.c_float), ("ratio_factor", C.c_float), ("merge_rule", C.c_int32)]


class _Result(C.Structure):   # uh_newpoints_result
    _fields_ = [("n_total", C.c_int32), ("status", VP), ("xyz_cam", VP), ("n_new", C.c_int32), ("n_obs", C.c_int32), ("kp_idx", VP),
                ("xyz_global", VP), ("distance", VP), ("chosen_pair", VP), ("chosen_match", VP), ("obs_ptr", VP), ("obs_pair", VP),
                ("obs_kpt", VP)]


def _declare(L, sig):
    sig("uh_newpoints_create", I, VP, C.POINTER(VP))
    sig("uh_newpoints_destroy", None, VP)
    sig("uh_newpoints_run", I, VP, C.POINTER(_Args), C.POINTER(_Result))
    sig("uh_fundamental_12", I, VP, VP, VP, VP)


_lib._EXTRA_DECLS.append(_declare)


def fundamental_12(intr4_train, intr4_query, RT) -> np.ndarray:
    """uh_fundamental_12: getFund12's F12 (3, 3) float32 for a (train, query) pair; RT = query.pose_f2g * train.pose_f2g.inv().  Host only."""
    a = np.ascontiguousarray(intr4_train, np.float32).reshape(4)
    b = np.ascontiguousarray(intr4_query, np.float32).reshape(4)
    rt = np.ascontiguousarray(RT, np.float32).reshape(16)
    out = np.zeros((3, 3), np.float32)
    check(lib().uh_fundamental_12(np_ptr(a), np_ptr(b), np_ptr(rt), np_ptr(out)))
    return out


def _copy(ptr, count, dtype, shape=None):
    if count == 0:
        return np.zeros((0,) + tuple(shape[1:]) if shape else (0,), dtype)
    a = np.frombuffer((C.c_char * (count * np.dtype(dtype).itemsize)).from_address(ptr), dtype, count).copy()
    return a.reshape(shape) if shape else a


class NewPoints:
    def __init__(self, ctx: _lib.Context):
        self.ctx = ctx
        self._h = VP()
        check(lib().uh_newpoints_create(ctx.handle, C.byref(self._h)))

    def run(self, new_kf, pairs, max_chi2=5.998, ratio_factor=1.5 * 1.2, merge_rule=MERGE_SMALLEST_OCTAVE, n_kpts=None):
        """new_kf: dict(intr4, scale_factors, pt (n, 2), octave (n), pose_g2f (4, 4), cam_center (3)); pairs: list of dict(RT (4, 4), intr4,
        scale_factors, cam_center, pt, octave, matches (DMATCH_DTYPE: queryIdx = the neighbour's keypoint, trainIdx = the new keyframe's)).
        Arrays are converted, never range-checked here: that is the library's part (n_kpts overrides the new keyframe's count for its tests).
        Returns dict(status (n_total), xyz_cam (n_total, 3), pair_offset (n_pairs + 1), n_new, kp_idx, xyz_global (n_new, 3), distance,
        chosen_pair, chosen_match, obs_ptr (n_new + 1), obs_pair, obs_kpt): copies, valid after the next run."""
        keep = []

        def arr(x, dt, shape=None):
            a = np.ascontiguousarray(x, dt)
            if shape is not None:
                a = a.reshape(shape)
            keep.append(a)
            return a

        ps = (_Pair * max(len(pairs), 1))()
        for j, p in enumerate(pairs):
            q = ps[j]
            q.RT[:] = arr(p["RT"], np.float32, 16).tolist()
            q.intr4[:] = arr(p["intr4"], np.float32, 4).tolist()
            q.cam_center[:] = arr(p["cam_center"], np.float32, 3).tolist()
            sf, pt, oc, m = arr(p["scale_factors"], np.float32), arr(p["pt"], np.float32, (-1, 2)), arr(p["octave"], np.int32), arr(p["matches"], DMATCH_DTYPE)
            q.n_levels, q.scale_factors = len(sf), np_ptr(sf)
            q.n_kpts, q.pt, q.octave = len(oc), np_ptr(pt), np_ptr(oc)
            q.n_matches, q.matches = len(m), np_ptr(m)
        a = _Args()
        a.intr4[:] = arr(new_kf["intr4"], np.float32, 4).tolist()
        a.pose_g2f[:] = arr(new_kf["pose_g2f"], np.float32, 16).tolist()
        a.cam_center[:] = arr(new_kf["cam_center"], np.float32, 3).tolist()
        sf, pt, oc = arr(new_kf["scale_factors"], np.float32), arr(new_kf["pt"], np.float32, (-1, 2)), arr(new_kf["octave"], np.int32)
        a.n_levels, a.scale_factors = len(sf), np_ptr(sf)
        a.n_kpts, a.pt, a.octave = (len(oc) if n_kpts is None else int(n_kpts)), np_ptr(pt), np_ptr(oc)
        a.n_pairs, a.pairs = len(pairs), C.cast(ps, VP)
        a.max_chi2, a.ratio_factor, a.merge_rule = float(max_chi2), float(ratio_factor), int(merge_rule)
        r = _Result()
        check(lib().uh_newpoints_run(self._h, C.byref(a), C.byref(r)))
        n, nn, no = r.n_total, r.n_new, r.n_obs
        return dict(status=_copy(r.status, n, np.uint8), xyz_cam=_copy(r.xyz_cam, 3 * n, np.float32, (-1, 3)),
                    pair_offset=np.cumsum([0] + [len(p["matches"]) for p in pairs]).astype(np.int64), n_new=int(nn),
                    kp_idx=_copy(r.kp_idx, nn, np.int32), xyz_global=_copy(r.xyz_global, 3 * nn, np.float32, (-1, 3)),
                    distance=_copy(r.distance, nn, np.float32), chosen_pair=_copy(r.chosen_pair, nn, np.int32),
                    chosen_match=_copy(r.chosen_match, nn, np.int32), obs_ptr=_copy(r.obs_ptr, nn + 1, np.int32),
                    obs_pair=_copy(r.obs_pair, no, np.int32), obs_kpt=_copy(r.obs_kpt, no, np.int32))

    def close(self):
        if self._h:
            lib().uh_newpoints_destroy(self._h)
            self._h = VP()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
