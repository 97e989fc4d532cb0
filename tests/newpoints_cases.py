"""Constructed problems for the new-map-point stage, shared by the host test (which fixes them against the oracle alone) and the GPU
test: one match per refusal branch of Triangulate / the scale-ratio check, and the merge cases."""
from __future__ import annotations

import numpy as np

import newpoints_synth as S

f32 = np.float32
I3 = np.zeros(3)


def _two_view(Xg, c2, rv2=I3, c1=I3, oct1=2, oct2=2, d1=(0, 0), d2=(0, 0)):
    """One point (global coordinates), the new keyframe at c1 looking down +z, one neighbour at c2 turned by rv2; d1 / d2 are pixel
    offsets added to the exact projections.  Two keypoints per frame: index 1 is the match, index 0 a bystander."""
    p1, p2 = S.pose(I3, c1), S.pose(rv2, c2)
    x1 = S.project(p1, S.INTR, [Xg])[0] + np.asarray(d1, float)
    x2 = S.project(p2, S.INTR, [Xg])[0] + np.asarray(d2, float)
    kf = S.make_new_kf(p1, [[5, 5], x1], [0, oct1])
    pair = S.make_pair(kf, p2, [[7, 7], x2], [0, oct2], [(1, 1, 33.0)])
    return kf, [pair]


def _inf_keypoint():
    kf, pairs = _two_view([0.3, -0.2, 5], [1, 0, 0])
    kf["pt"][1, 0] = np.inf
    return kf, pairs


def _opposite_rays():
    # no geometry behind it: a neighbour turned by 80 degrees, keypoints at opposite image edges -> the rays are more than 90 degrees apart
    p1, p2 = S.pose(I3, I3), S.pose([0, -np.deg2rad(80), 0], [1, 0, 0])
    kf = S.make_new_kf(p1, [[5, 5], [10, 250]], [0, 2])
    return kf, [S.make_pair(kf, p2, [[7, 7], [630, 250]], [0, 2], [(1, 1, 33.0)])]


BIG = 1e8   # float32 spacing 8 there: a point within 4 of the camera centre IS the camera centre after rounding

# name -> (builder, the status code the oracle must report for the one match)
BRANCH = {
    "accepted": (lambda: _two_view([0.3, -0.2, 5], [1, 0, 0]), 0),
    "parallax_below_1p1_deg": (lambda: _two_view([0.3, -0.2, 200], [1, 0, 0]), 1),          # atan(1 / 200) = 0.29 degrees
    "rays_more_than_90_deg_apart": (_opposite_rays, 1),
    "behind_camera_1": (lambda: _two_view([0.3, -0.2, -5], [1, 0, 0]), 4),
    "behind_camera_2_only": (lambda: _two_view([1.0, 0.0, 4], [0.3, 0, 6]), 5),
    "gross_error_image_1": (lambda: _two_view([0.3, -0.2, 5], [1, 0, 0], d1=(0, 40)), 6),
    # the null vector spreads a one-sided error over both images, and image 1 is tested first: its keypoint sits on octave 7
    # (weight 1 / 3.58^2), the neighbour's on octave 0, so the same residual passes in image 1 and fails in image 2
    "gross_error_image_2": (lambda: _two_view([0.3, -0.2, 5], [1, 0, 0], oct1=7, oct2=0, d2=(0, 9)), 7),
    "on_camera_centre_after_rounding": (lambda: _two_view([BIG + 3.9, BIG + 3.9, BIG + 3.9], [BIG + 8, BIG, BIG], c1=[BIG, BIG, BIG]), 8),
    "octave_ratio_low_side": (lambda: _two_view([0.5, -0.2, 5], [1, 0, 0], oct1=7, oct2=0), 9),    # ratioDist * 1.8 < 3.58
    "octave_ratio_high_side": (lambda: _two_view([0.5, -0.2, 5], [1, 0, 0], oct1=0, oct2=7), 9),   # ratioDist > 0.28 * 1.8
    "inf_keypoint": (_inf_keypoint, 3),
}


def merge_scene():
    """Keypoints of the new keyframe: 0 seen from three neighbours on octaves (2, 1, 1); 1 seen from three on equal octaves; 2 with one
    candidate, which is refused (gross pixel error); 3 seen from the last neighbour only; 4 unmatched.
    Returns (kf, pairs, expectations)."""
    X = np.array([[0.3, -0.2, 5.0], [-0.6, 0.4, 6.0], [0.9, 0.1, 4.5], [-0.2, -0.5, 5.5]])
    p1 = S.pose(I3, I3)
    kf = S.make_new_kf(p1, np.vstack([S.project(p1, S.INTR, X), [[100, 100]]]), [1, 3, 2, 2, 0])
    centres = [[1, 0, 0], [-1, 0.2, 0], [0, 1, 0.1]]
    octs = [[2, 3, 2, 2], [1, 3, 2, 2], [1, 3, 2, 2]]
    pairs = []
    for j in range(3):
        p2 = S.pose([0, 0.02 * j, 0.01], centres[j])
        pt = S.project(p2, S.INTR, X)
        rows = [(0, 0, 40.0 + j), (1, 1, 50.0 + j)]
        if j == 0:
            pt[2, 1] += 60.0            # keypoint 2's only candidate: refused
            rows.append((2, 2, 60.0))
        if j == 2:
            rows.append((3, 3, 70.0))
        # the neighbour's keypoints are stored in reverse, so that queryIdx != trainIdx
        n = len(pt)
        rows = [(n - 1 - q, t, d) for (q, t, d) in rows]
        pairs.append(S.make_pair(kf, p2, pt[::-1], octs[j][::-1], rows))
    expect = dict(kp_idx=[0, 1, 3], chosen_pair=[1, 0, 2], chosen_pair_as_compiled=[2, 2, 2], obs_pair=[-1, 0, 1, 2, -1, 0, 1, 2, -1, 2],
                  obs_ptr=[0, 4, 8, 10])
    return kf, pairs, expect
