"""Constructed cases of the relocalisation RANSAC and the shared, cached oracle results of its scenes: the CPU test fixes every case
against the numpy oracle alone, the GPU test compares the device with the same objects."""
from __future__ import annotations

import functools

import numpy as np

import pnp_ransac_oracle as O
import pnp_ransac_synth as S

f32 = np.float32


@functools.lru_cache(maxsize=None)
def scene_and_oracle(name):
    pr = S.parity_scene(name) if name in S.PARITY else S.planted_scene(name)
    return pr, O.run(pr)


def _exact_scene(seed, n):
    """n noise-free matches of a planted pose (pixels rounded to float32 only)."""
    pr = S.scene(seed, n, 1, outliers=0.0)
    pr["kp"] = np.ascontiguousarray(S.project(pr["planted_R"], pr["planted_t"], pr["intr"], pr["p3d"].astype(np.float64)).astype(f32))
    return pr


@functools.lru_cache(maxsize=None)
def repeated_sample():
    """The sample of iteration 2 repeated bit for bit at iteration 7, both with the largest count: best_iter = 2.  Every other iteration
    holds a gross outlier among its first three points."""
    pr = S.scene(410, 200, 10, outliers=0.3)
    good = np.nonzero(pr["planted_inlier"])[0]
    bad = np.nonzero(~pr["planted_inlier"])[0]
    smp = np.zeros((10, 4), np.int32)
    for it in range(10):
        smp[it] = [bad[it], good[3 * it], good[3 * it + 1], good[3 * it + 2]]
    smp[2] = smp[7] = [good[40], good[47], good[55], good[61]]
    pr["samples"] = smp
    return pr, O.run(pr)


@functools.lru_cache(maxsize=None)
def collinear():
    """Samples 0-2 of every hypothesis are three points of one line (exact in float32): every iteration is skipped."""
    pr = S.scene(420, 40, 6, outliers=0.0)
    p = pr["p3d"].copy()
    p[0], p[1], p[2], p[3] = (0, 0, 5), (1, 0, 5), (2, 0, 5), (4, 0, 5)
    pr["p3d"] = p
    pr["samples"] = np.array([[0, 1, 2, 9], [2, 1, 0, 10], [1, 3, 0, 11], [3, 2, 1, 12], [0, 2, 3, 13], [3, 0, 1, 5]], np.int32)
    return pr, O.run(pr)


@functools.lru_cache(maxsize=None)
def best_of_three():
    """Four matches, the fourth a gross outlier, one iteration: its three sample points are the only inliers — ok = 0, and the pose is
    overwritten all the same (the reference calls setRT before it returns false)."""
    pr = _exact_scene(430, 4)
    pr["kp"][3] += f32(80)
    pr["samples"] = np.array([[0, 1, 2, 3]], np.int32)
    return pr, O.run(pr)


SPECIAL_EXPECT = [True, True, True, True, True, False, False]


@functools.lru_cache(maxsize=None)
def special_points():
    """Four exact matches (the sample) and three more: [4] a point BEHIND the camera whose projection falls on its keypoint (counts:
    the reference has no test of the depth's sign), [5] a point on the camera plane (does not count), [6] a point that reprojects
    exactly but is seen at a view cosine of 0.49 (rejected)."""
    pr = _exact_scene(440, 7)
    R, t = pr["planted_R"], pr["planted_t"]
    centre = -R.T @ t
    Xc = pr["p3d"].astype(np.float64) @ R.T + t
    p, nrm, kp = pr["p3d"].copy(), pr["normal"].copy(), pr["kp"].copy()
    p[4] = (R.T @ (-Xc[4] - t)).astype(f32)               # mirrored through the centre: same pixel, negative depth
    p[5] = (R.T @ (np.array([Xc[5, 0], Xc[5, 1], 0.0]) - t)).astype(f32)
    for i in (4, 5):
        d = centre - p[i].astype(np.float64)
        nrm[i] = (d / np.linalg.norm(d)).astype(f32)
    d = centre - p[6].astype(np.float64)
    d /= np.linalg.norm(d)
    o = np.cross(d, [0.3, -0.5, 0.8])
    o /= np.linalg.norm(o)
    nrm[6] = (0.49 * d + np.sqrt(1 - 0.49 ** 2) * o).astype(f32)
    pr["p3d"], pr["normal"], pr["kp"] = np.ascontiguousarray(p), np.ascontiguousarray(nrm), np.ascontiguousarray(kp)
    pr["samples"] = np.array([[0, 1, 2, 3]], np.int32)
    return pr, O.run(pr)


def band_pairs(h):
    """number of matches of a hypothesis inside the band of a threshold"""
    return int((h["margin"] < O.NEAR).sum())


TOL = 1e-6   # the project's bar for PnP and BA against a reference
# "within the noise" of a planted pose: a pose that brings every planted inlier, spread over the whole image, within the gate of
# sqrt(5.99) = 2.45 px of its keypoint is rotated by at most about 2.45 / fx = 3.4e-3 rad against the planted one and shifted by at most
# about that angle times the largest depth (10): bars of three times those figures (max |R - R0|, max |t - t0|)
POSE_BARS = (1e-2, 1e-1)


def planted_pose_error(pr, rt6):
    R = S.rodrigues(np.asarray(rt6[:3], np.float64))
    dR, dt = float(np.abs(R - pr["planted_R"]).max()), float(np.abs(np.asarray(rt6[3:], np.float64) - pr["planted_t"]).max())
    print(f"pose against the planted one: rotation {dR:.3g}, translation {dt:.3g}")
    return dR, dt


def rt6_must_equal(h, got_double):
    """Which of the six components of a hypothesis' rt6 must be equal BIT FOR BIT between the oracle and an implementation whose chosen
    (rvec, tvec) in double is got_double.  Two doubles round to different floats only if a float rounding tie lies between them, so a
    component is exempt exactly when the oracle's double lies within |difference| + 1e-3 float ulp of such a tie; everywhere else the
    bits are asserted.  Returns the boolean mask (True = must be equal)."""
    od = np.asarray(h["rvec_tvec"], np.float64)
    of = np.asarray(h["rt6"], np.float32)
    ulp = np.spacing(np.abs(of)).astype(np.float64)
    to_tie = np.abs(np.abs(od - of.astype(np.float64)) - 0.5 * ulp)
    return to_tie > np.abs(np.asarray(got_double, np.float64) - od) + 1e-3 * ulp
