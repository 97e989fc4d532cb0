"""Stereo / RGB-D frames: Frame::depth per keypoint on the device (uh_stereo_depth*, uh_rgbd_depth*, uh_orb_extract_stereo / _rgbd) —
FrameExtractor::processStereo and process_rgbd (src/utils/frameextractor.cpp from :1419) for kptImageScaleFactor == 1.  See
include/ucoslam_hip.h for the contract, csrc/stereo.hip for the kernels, csrc/stereo_math.hpp for the arithmetic."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import I, SZ, VP, check, dev_ptr, lib, np_ptr
from .orb import KEYPOINT_DTYPE


class _Args(C.Structure):   # uh_stereo_args
    _fields_ = [("left", VP), ("left_stride", SZ), ("right", VP), ("right_stride", SZ), ("cols", C.c_int32), ("rows", C.c_int32),
                ("right_cols", C.c_int32), ("right_rows", C.c_int32), ("n_left", C.c_int32), ("left_und_kpts", VP), ("left_desc", VP),
                ("n_right", C.c_int32), ("right_kpts", VP), ("right_desc", VP), ("bl", C.c_float), ("fx", C.c_float), ("max_desc_dist", C.c_float)]


class _Right(C.Structure):   # uh_stereo_right
    _fields_ = [("kps", VP), ("desc", VP), ("n", C.c_int32)]


def _declare(L, sig):
    sig("uh_stereo_depth", I, VP, C.POINTER(_Args), VP, VP)
    sig("uh_stereo_depth_dev", I, VP, C.POINTER(_Args), VP, VP)
    sig("uh_stereo_depth_host", I, C.POINTER(_Args), VP, VP)
    sig("uh_rgbd_depth", I, VP, VP, C.c_int32, VP, C.c_int32, C.c_int32, SZ, C.c_float, VP)
    sig("uh_rgbd_depth_host", I, VP, C.c_int32, VP, C.c_int32, C.c_int32, SZ, C.c_float, VP)
    sig("uh_orb_set_stereo", I, VP, C.c_float, C.c_float)
    sig("uh_orb_extract_stereo", I, VP, VP, VP, I, I, SZ, I, VP, VP, VP, VP, I, C.POINTER(I), VP, C.POINTER(_Right))
    sig("uh_orb_extract_rgbd", I, VP, VP, I, I, SZ, I, VP, SZ, C.c_float, VP, VP, VP, VP, I, C.POINTER(I), VP)


_lib._EXTRA_DECLS.append(_declare)


def _gray(img):
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 2:
        raise _lib.UcoslamHipError(_lib.UH_EINVAL, "image must be CV_8UC1 (2-D uint8)")
    return a if a.strides[1] == 1 else np.ascontiguousarray(a)


def _host_args(left, right, left_und_kpts, left_desc, right_kpts, right_desc, bl, fx, max_desc_dist, n_left=None, n_right=None):
    """Arrays are converted, never range-checked here: that is the library's part (n_left / n_right override the counts for its tests)."""
    L, R = _gray(left), _gray(right)
    lk, rk = np.ascontiguousarray(left_und_kpts, KEYPOINT_DTYPE), np.ascontiguousarray(right_kpts, KEYPOINT_DTYPE)
    ld, rd = np.ascontiguousarray(left_desc, np.uint8).reshape(-1, 32), np.ascontiguousarray(right_desc, np.uint8).reshape(-1, 32)
    a = _Args()
    a.left, a.left_stride, a.right, a.right_stride = np_ptr(L), L.strides[0], np_ptr(R), R.strides[0]
    a.rows, a.cols = L.shape
    a.right_rows, a.right_cols = R.shape
    a.n_left, a.left_und_kpts, a.left_desc = (len(lk) if n_left is None else int(n_left)), np_ptr(lk), np_ptr(ld)
    a.n_right, a.right_kpts, a.right_desc = (len(rk) if n_right is None else int(n_right)), np_ptr(rk), np_ptr(rd)
    a.bl, a.fx, a.max_desc_dist = float(bl), float(fx), float(max_desc_dist)
    return a, (L, R, lk, rk, ld, rd), len(lk)


def stereo_depth_host(left, right, left_und_kpts, left_desc, right_kpts, right_desc, bl, fx, max_desc_dist, **kw):
    """uh_stereo_depth_host (CPU, no GPU): -> (depth float32 (n_left), match int32 (n_left): right index or -1)."""
    a, keep, n = _host_args(left, right, left_und_kpts, left_desc, right_kpts, right_desc, bl, fx, max_desc_dist, **kw)
    depth, match = np.zeros(max(n, 1), np.float32), np.full(max(n, 1), -1, np.int32)
    check(lib().uh_stereo_depth_host(C.byref(a), np_ptr(depth), np_ptr(match)))
    return depth[:n], match[:n]


def stereo_depth(ctx: _lib.Context, left, right, left_und_kpts, left_desc, right_kpts, right_desc, bl, fx, max_desc_dist, **kw):
    """uh_stereo_depth: the same on the device from host arrays (one wait)."""
    a, keep, n = _host_args(left, right, left_und_kpts, left_desc, right_kpts, right_desc, bl, fx, max_desc_dist, **kw)
    depth, match = np.zeros(max(n, 1), np.float32), np.full(max(n, 1), -1, np.int32)
    check(lib().uh_stereo_depth(ctx.handle, C.byref(a), np_ptr(depth), np_ptr(match)))
    return depth[:n], match[:n]


def stereo_depth_dev(ctx: _lib.Context, left, right, left_und_kpts, left_desc, right_kpts, right_desc, bl, fx, max_desc_dist, want_match=True):
    """uh_stereo_depth_dev: torch CUDA tensors in (uint8 images H x W, keypoints as uint8 (n, 28) or float32 (n, 7) views of cv::KeyPoint records,
    descriptors uint8 (n, 32)), torch tensors out; asynchronous on the context stream."""
    import torch

    a = _Args()
    a.left, a.left_stride, a.right, a.right_stride = dev_ptr(left), left.stride(0), dev_ptr(right), right.stride(0)
    a.rows, a.cols = left.shape
    a.right_rows, a.right_cols = right.shape
    nl, nr = int(left_und_kpts.shape[0]), int(right_kpts.shape[0])
    a.n_left, a.left_und_kpts, a.left_desc = nl, dev_ptr(left_und_kpts), dev_ptr(left_desc)
    a.n_right, a.right_kpts, a.right_desc = nr, dev_ptr(right_kpts), dev_ptr(right_desc)
    a.bl, a.fx, a.max_desc_dist = float(bl), float(fx), float(max_desc_dist)
    depth = torch.zeros(max(nl, 1), dtype=torch.float32, device=left.device)
    match = torch.full((max(nl, 1),), -1, dtype=torch.int32, device=left.device) if want_match else None
    check(lib().uh_stereo_depth_dev(ctx.handle, C.byref(a), dev_ptr(depth), dev_ptr(match) if want_match else None))
    return depth[:nl], (match[:nl] if want_match else None)


def _depth_img(d):
    a = np.asarray(d)
    if a.dtype != np.uint16 or a.ndim != 2:
        raise _lib.UcoslamHipError(_lib.UH_EINVAL, "depth image must be CV_16UC1 (2-D uint16)")
    return a if a.strides[1] == 2 else np.ascontiguousarray(a)


def rgbd_depth_host(kpts, depth_img, depth_scale):
    """uh_rgbd_depth_host: process_rgbd's gather on the CPU -> depth float32 (n)."""
    k, D = np.ascontiguousarray(kpts, KEYPOINT_DTYPE), _depth_img(depth_img)
    out = np.zeros(max(len(k), 1), np.float32)
    check(lib().uh_rgbd_depth_host(np_ptr(k), len(k), np_ptr(D), D.shape[1], D.shape[0], D.strides[0], float(depth_scale), np_ptr(out)))
    return out[: len(k)]


def rgbd_depth(ctx: _lib.Context, kpts, depth_img, depth_scale):
    """uh_rgbd_depth: the same on the device."""
    k, D = np.ascontiguousarray(kpts, KEYPOINT_DTYPE), _depth_img(depth_img)
    out = np.zeros(max(len(k), 1), np.float32)
    check(lib().uh_rgbd_depth(ctx.handle, np_ptr(k), len(k), np_ptr(D), D.shape[1], D.shape[0], D.strides[0], float(depth_scale), np_ptr(out)))
    return out[: len(k)]


def _frame_img(image):
    img = np.asarray(image)
    cn = 1 if img.ndim == 2 else img.shape[2]
    if img.dtype != np.uint8 or img.ndim not in (2, 3) or cn not in (1, 3, 4):
        raise _lib.UcoslamHipError(_lib.UH_EINVAL, "image must be uint8, H x W [x 3 | x 4]")
    if img.strides[-1] != 1 or (img.ndim == 3 and img.strides[1] != cn):
        img = np.ascontiguousarray(img)
    return img, cn


def set_stereo(orb, bl: float, max_desc_dist: float):
    """uh_orb_set_stereo on an ORBextractor: ImageParams::bl and Params::maxDescDistance."""
    check(lib().uh_orb_set_stereo(orb._h, float(bl), float(max_desc_dist)))
    return orb


def extract_stereo(orb, left, right, frame=None, want_right=False, cap=None):
    """uh_orb_extract_stereo -> dict(kps, desc, und_xy, depth[, right_kps, right_desc]); `frame`: a DeviceFrame or None."""
    L, cn = _frame_img(left)
    R, cn_r = _frame_img(right)
    if L.shape != R.shape or L.strides != R.strides:
        raise _lib.UcoslamHipError(_lib.UH_EINVAL, f"uh_orb_extract_stereo: left image {L.shape} but right image {R.shape}")
    maxk = max(lib().uh_orb_max_keypoints(orb._h), 1)
    cap = maxk if cap is None else int(cap)
    kps, desc = np.zeros(max(cap, 1), KEYPOINT_DTYPE), np.zeros((max(cap, 1), 32), np.uint8)
    und, depth = np.zeros((max(cap, 1), 2), np.float32), np.zeros(max(cap, 1), np.float32)
    n = C.c_int(0)
    ro = _Right()
    if want_right:
        rk, rd = np.zeros(maxk, KEYPOINT_DTYPE), np.zeros((maxk, 32), np.uint8)
        ro.kps, ro.desc = np_ptr(rk), np_ptr(rd)
    check(lib().uh_orb_extract_stereo(orb._h, np_ptr(L), np_ptr(R), L.shape[1], L.shape[0], L.strides[0], cn, np_ptr(kps), np_ptr(desc), np_ptr(und),
                                      np_ptr(depth), cap, C.byref(n), frame._h if frame is not None else None, C.byref(ro) if want_right else None))
    out = dict(kps=kps[: n.value].copy(), desc=desc[: n.value].copy(), und_xy=und[: n.value].copy(), depth=depth[: n.value].copy())
    if want_right:
        out.update(right_kps=rk[: ro.n].copy(), right_desc=rd[: ro.n].copy())
    return out


def extract_rgbd(orb, image, depth_img, depth_scale, frame=None, undistorted=True):
    """uh_orb_extract_rgbd -> dict(kps, desc, und_xy, depth)."""
    img, cn = _frame_img(image)
    D = _depth_img(depth_img)
    if D.shape != img.shape[:2]:
        raise _lib.UcoslamHipError(_lib.UH_EINVAL, f"uh_orb_extract_rgbd: image {img.shape[:2]} but depth image {D.shape}")
    cap = max(lib().uh_orb_max_keypoints(orb._h), 1)
    kps, desc = np.zeros(cap, KEYPOINT_DTYPE), np.zeros((cap, 32), np.uint8)
    und, depth = (np.zeros((cap, 2), np.float32) if undistorted else None), np.zeros(cap, np.float32)
    n = C.c_int(0)
    check(lib().uh_orb_extract_rgbd(orb._h, np_ptr(img), img.shape[1], img.shape[0], img.strides[0], cn, np_ptr(D), D.strides[0], float(depth_scale),
                                    np_ptr(kps), np_ptr(desc), np_ptr(und) if undistorted else None, np_ptr(depth), cap, C.byref(n),
                                    frame._h if frame is not None else None))
    return dict(kps=kps[: n.value].copy(), desc=desc[: n.value].copy(), und_xy=(und[: n.value].copy() if undistorted else None), depth=depth[: n.value].copy())
