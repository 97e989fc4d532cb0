#!/usr/bin/env python3
"""Times the new-map-point stage (uh_newpoints_run): 20 neighbours x 1 000 matches on 2 000 + 20 x 2 000 keypoints, host arrays in,
pinned host results out (the call ends in a stream synchronise), 200 repetitions after a warm-up; reports the median and the spread.
A second leg times the ctypes mirror's own packing and copying apart from the library call.

For scale only, the numpy oracle of the tests is timed on the same input.  THAT IS NOT THE REFERENCE'S TIME: the reference's
Triangulate (cv::SVD per match on one core, OpenMP over the neighbours) cannot be built without OpenCV and was not measured.

    python scripts/time_newpoints.py [--out profiles/newpoints_time.txt] [--reps 200] [--pairs 20] [--matches 1000] [--kpts 2000]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/time_newpoints.py --reps 50      (the per-kernel split, a run of its own)"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--matches", type=int, default=1000)
    ap.add_argument("--kpts", type=int, default=2000)
    a = ap.parse_args()
    import torch

    import __graft_entry__  # noqa: F401  (puts the package on the path)
    import newpoints_oracle as O
    import newpoints_synth as S
    import ucoslam_cv3_amd as u
    from ucoslam_cv3_amd import newpoints as npm
    from ucoslam_cv3_amd._lib import check, lib

    assert torch.cuda.is_available(), "needs a GPU: a time taken anywhere else says nothing"
    kf, pairs = S.scene(4242, [a.matches] * a.pairs, a.kpts, a.kpts)
    ctx = u.Context(0, torch.cuda.current_stream().cuda_stream)
    h = npm.NewPoints(ctx)
    for _ in range(10):
        out = h.run(kf, pairs, ratio_factor=S.RATIO_FACTOR)

    # leg 1: the mirror, as a Python host pays for it
    t_mirror = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        out = h.run(kf, pairs, ratio_factor=S.RATIO_FACTOR)
        t_mirror.append(1e6 * (time.perf_counter() - t0))

    # leg 2: the library call alone on prepared argument structs (what a C++ host pays): validation, packing, upload, two kernels,
    # download, wait
    keep = []
    ps = (npm._Pair * a.pairs)()
    for j, p in enumerate(pairs):
        arrs = [np.ascontiguousarray(p[k], dt) for k, dt in (("scale_factors", np.float32), ("pt", np.float32), ("octave", np.int32), ("matches", npm.DMATCH_DTYPE))]
        keep += arrs
        q = ps[j]
        q.RT[:] = np.asarray(p["RT"], np.float32).ravel().tolist()
        q.intr4[:] = np.asarray(p["intr4"], np.float32).tolist()
        q.cam_center[:] = np.asarray(p["cam_center"], np.float32).tolist()
        q.n_levels, q.scale_factors = len(arrs[0]), npm.np_ptr(arrs[0])
        q.n_kpts, q.pt, q.octave = len(arrs[2]), npm.np_ptr(arrs[1]), npm.np_ptr(arrs[2])
        q.n_matches, q.matches = len(arrs[3]), npm.np_ptr(arrs[3])
    args = npm._Args()
    args.intr4[:] = kf["intr4"].tolist()
    args.pose_g2f[:] = kf["pose_g2f"].ravel().tolist()
    args.cam_center[:] = kf["cam_center"].tolist()
    args.n_levels, args.scale_factors = len(kf["scale_factors"]), npm.np_ptr(kf["scale_factors"])
    args.n_kpts, args.pt, args.octave = len(kf["octave"]), npm.np_ptr(kf["pt"]), npm.np_ptr(kf["octave"])
    args.n_pairs, args.pairs = a.pairs, C.cast(ps, C.c_void_p)
    args.max_chi2, args.ratio_factor, args.merge_rule = 5.998, S.RATIO_FACTOR, 0
    res = npm._Result()
    run = lib().uh_newpoints_run
    for _ in range(10):
        check(run(h._h, C.byref(args), C.byref(res)))
    t_call = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        rc = run(h._h, C.byref(args), C.byref(res))
        t_call.append(1e6 * (time.perf_counter() - t0))
        check(rc)
    assert res.n_new == out["n_new"]

    t0 = time.perf_counter()
    ref = O.run(kf, pairs, ratio_factor=S.RATIO_FACTOR)
    t_oracle = 1e3 * (time.perf_counter() - t0)
    assert ref["n_new"] == out["n_new"] or (ref["margin"] < O.NEAR).any()

    def line(name, t):
        t = np.sort(np.asarray(t))
        return (f"{name:<46s} median {np.median(t):8.1f} us   p10 {t[len(t) // 10]:8.1f}   p90 {t[(9 * len(t)) // 10]:8.1f}   min {t[0]:8.1f}   "
                f"max {t[-1]:8.1f}   ({len(t)} runs)")

    n_total = len(out["status"])
    lines = [f"new map points: {a.pairs} pairs x {a.matches} matches = {n_total} matches, {a.kpts} + {a.pairs} x {a.kpts} keypoints; "
             f"{out['n_new']} new points, {len(out['obs_pair'])} observations; device: {torch.cuda.get_device_name(0)}",
             "host arrays in, pinned host results out, every call ends in a stream synchronise; after 10 warm-up calls",
             line("uh_newpoints_run (prepared argument structs)", t_call),
             line("NewPoints.run (ctypes mirror, packs and copies)", t_mirror),
             f"for scale only, the numpy oracle of the tests on the same input, one run: {t_oracle:.1f} ms.  This is NOT the reference's time: "
             "the reference's Triangulate (cv::SVD per match) cannot be built here and was not measured."]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    h.close()


if __name__ == "__main__":
    main()
