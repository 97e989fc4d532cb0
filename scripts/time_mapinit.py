#!/usr/bin/env python3
"""Times the map initialiser (uh_mapinit_run): ONE call at n = 1000 matches, 200 iterations, host arrays in and host arrays out.

  1. Wall time of the synchronous library call on prepared arguments (it ends in a stream synchronise), median and spread over --reps
     calls after a warm-up, alternating with
  2. uh_mapinit_run_host on one core of the same machine.  THIS IS THE LIBRARY'S OWN HOST FORM, NOT THE REFERENCE: MapInitializer needs
     OpenCV and cannot be built here; nobody has measured it.
  3. In a pass of its own, with the context's event profiling on: the two kernels' own times (HIP events around each launch).

The timed window is --reps calls of about a millisecond each: 3000 by default, some three seconds per scene after 200 warm-up calls.
--calls-only runs the warm-up and the calls and nothing else, for a kernel trace in a run of its own:

    python scripts/time_mapinit.py [--out profiles/mapinit_time.txt] [--reps 3000]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/time_mapinit.py --calls-only --reps 500"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(t):
    t = np.sort(np.array(t))
    return f"median {np.median(t):9.1f} us   p10 {t[len(t) // 10]:9.1f}   p90 {t[(9 * len(t)) // 10]:9.1f}   min {t[0]:9.1f}   (n = {len(t)})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3000)
    ap.add_argument("--calls-only", action="store_true")
    a = ap.parse_args()
    import torch

    import mapinit_cases as MC
    import ucoslam_cv3_amd as u
    from ucoslam_cv3_amd import mapinit as MI
    from ucoslam_cv3_amd._lib import check, lib

    assert torch.cuda.is_available(), "needs a GPU: a time taken anywhere else says nothing"
    ctx = u.Context(0, torch.cuda.current_stream().cuda_stream)
    lines = ["map initialiser timing (scripts/time_mapinit.py): wall time of the synchronous library call on prepared arguments, microseconds", ""]
    for name in ("general_1000", "plane_1000"):
        sc = MC.scene(name)
        mi = MI.MapInit(ctx)
        call, _args, r, keep = mi.prepare(sc["intr"], sc["kp1"], sc["kp2"], sc["matches"])
        ah, rh, keeph = MI._pack(sc["intr"], sc["kp1"], sc["kp2"], sc["matches"], **MI._DEFAULTS)
        host = lambda: lib().uh_mapinit_run_host(C.byref(ah), C.byref(rh))   # noqa: E731
        for _ in range(200):
            check(call())
        if a.calls_only:
            for _ in range(a.reps):
                check(call())
            mi.close()
            continue
        check(host())
        assert r.ok == rh.ok == 1 and keep["po"].tobytes() == keeph["po"].tobytes() and keep["mo"].tobytes() == keeph["mo"].tobytes(), "device form != host form"
        td, th = [], []
        for i in range(a.reps):   # alternating: both see the same machine (the host form every tenth round: it is the slow one)
            t0 = time.perf_counter(); call(); t1 = time.perf_counter()
            td.append(1e6 * (t1 - t0))
            if i % 10 == 0:
                t0 = time.perf_counter(); host(); th.append(1e6 * (time.perf_counter() - t0))
        ctx.prof_enable(True)
        ctx.prof_reset()
        for _ in range(50):
            check(call())
        ctx.synchronize()
        rep = ctx.prof_report()
        ctx.prof_enable(False)
        lines += [f"{name}: {len(sc['matches'])} matches, {len(sc['kp1'])} keypoints per frame, 200 iterations, model {r.model}, {r.n_out} points",
                  f"  uh_mapinit_run                    {stats(td)}",
                  f"  uh_mapinit_run_host, one core     {stats(th)}   <- the library's own host form, NOT the reference",
                  f"  host form / device form           {np.median(th) / np.median(td):.1f}"]
        for k, (calls, ms) in sorted(rep.items()):
            lines.append(f"  kernel {k:28s} {1e3 * ms / max(calls, 1):9.1f} us per launch   ({calls} launches, HIP events, a pass of its own)")
        lines.append("")
        mi.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(text + "\n")


if __name__ == "__main__":
    main()
