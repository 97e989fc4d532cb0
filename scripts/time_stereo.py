"""Per-frame cost of the stereo extraction at 1241 x 376 with the bench's extractor parameters (2000 features, 8 levels, 1.2):
  (a) uh_orb_extract_frame of the left image: the monocular cost
  (b) two such calls back to back (left, right): what a host pays today for the two extractions alone
  (c) uh_orb_extract_stereo: both extractions, row index, match, SAD refinement, one wait
  (d) the stereo kernels' own device time (uh_prof_report, in a run of its own with profiling on)
The forms alternate inside every round; a figure is the median over the rounds of each round's median call, the spread is the rounds'
min .. max.  --lib PATH times another build of the library (its monocular forms only with --mono-only: the parent commit has no stereo entry).

  python scripts/time_stereo.py [--rounds 7] [--calls 200] [--lib PATH] [--mono-only]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--mono-only", action="store_true")
    a = ap.parse_args()
    import torch

    import synth
    from ucoslam_cv3_amd import _lib

    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    if a.mono_only:   # a library without the stereo entry points: only the extractor's prototypes are declared
        from ucoslam_cv3_amd import orb as _orb

        _lib._EXTRA_DECLS[:] = [_orb._declare]
    from ucoslam_cv3_amd.orb import Camera, FeatParams, ORBextractor

    torch.cuda.set_device(0)
    ctx = _lib.Context(0, private=True)
    w, h = 1241, 376
    left, right = synth.frame(w, h, seed=5), synth.frame(w, h, seed=6, shift=(12, 0))
    ext = ORBextractor(ctx)
    ext.detectAndCompute(np.zeros((0, 0), np.uint8), None, FeatParams(2000, 8, 1.2))
    ext.setCamera(Camera(718.856, 718.856, 607.19, 185.22, ()))
    forms = {"a_mono": lambda: ext.extractFrame(left), "b_two_mono": lambda: (ext.extractFrame(left), ext.extractFrame(right))}
    if not a.mono_only:
        from ucoslam_cv3_amd.stereo import extract_stereo, set_stereo

        set_stereo(ext, 0.54, 50.0)
        forms["c_stereo"] = lambda: extract_stereo(ext, left, right)
    for f in forms.values():
        for _ in range(20):
            f()
    per_round = {k: [] for k in forms}
    for _ in range(a.rounds):
        for k, f in forms.items():
            ts = []
            for _ in range(a.calls):
                t0 = time.perf_counter()
                f()
                ts.append(time.perf_counter() - t0)
            per_round[k].append(float(np.median(ts)) * 1e3)
    print(f"library {_lib.LIB_PATH}")
    print(f"{w} x {h}, 2000 features, 8 levels; {a.rounds} rounds of {a.calls} calls per form, forms alternating; ms per call through the Python mirror")
    for k, v in per_round.items():
        print(f"  {k:11s} median {np.median(v):.4f}   rounds min {min(v):.4f} max {max(v):.4f}   spread {max(v) - min(v):.4f}")
    if not a.mono_only:
        n_prof = 50
        ctx.prof_enable(True)
        ctx.prof_reset()
        for _ in range(n_prof):
            r = forms["c_stereo"]()
        ctx.synchronize()
        rep = ctx.prof_report()
        ctx.prof_enable(False)
        print(f"  (d) device time per call over {n_prof} profiled calls ({len(r['kps'])} left keypoints, {int((r['depth'] != 0).sum())} with a depth), us:")
        tot = 0.0
        for name, (calls, ms) in sorted(rep.items()):
            us = ms * 1e3 / n_prof
            if name.startswith("st_"):
                tot += us
            print(f"      {name:24s} {calls / n_prof:4.1f} launches  {us:8.2f}")
        print(f"      the three stereo kernels together {tot:.2f}")


if __name__ == "__main__":
    main()
