#!/usr/bin/env python3
"""Times the loop-closure pose graph (uh_posegraph_optimize) on 100 / 400 / 1000 keyframes — fixed scale, the synthetic ring of
tests/posegraph_synth.py, host arrays in, host arrays out, median of repeated runs after a warm-up — beside the real g2o on one CPU core
(the driver tests/golden/posegraph_ref.cpp, where tests/golden/make_posegraph_golden.py has built it), and splits the device time into
its phases with the context's per-kernel event timing (a run of its own: the events serialise the stream).

    python scripts/time_posegraph.py [--out profiles/posegraph_time.txt] [--sizes 100,400,1000] [--reps 5]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="100,400,1000")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch

    import __graft_entry__  # noqa: F401  (puts the package on the path)
    import posegraph_synth
    import ucoslam_cv3_amd as u
    from ucoslam_cv3_amd.posegraph import PoseGraph

    assert torch.cuda.is_available(), "needs a GPU"
    ref = None
    try:
        import make_posegraph_golden as gen

        if os.path.exists(gen.LIB):
            ref = gen
    except Exception as e:   # the driver is optional
        print("no reference driver:", e)
    ctx = u.Context(0, torch.cuda.current_stream().cuda_stream)
    pg = PoseGraph(ctx)
    lines = [f"loop-closure pose graph, fixed scale, synthetic ring; device: {torch.cuda.get_device_name(0)}; median of {a.reps} after one warm-up",
             "keyframes edges n      iters trials | device ms (min .. max) | g2o ms, one core | g2o / device | phases of one run, ms"]
    for n in [int(s) for s in a.sizes.split(",")]:
        pr = posegraph_synth.posegraph_problem(n=n, seed=900 + n, fix_scale=True, skip2=8)
        args = (pr["poses"], pr["edge_i"], pr["edge_j"], None, pr["idx_new"], pr["idx_old"], pr["expected"], 1)
        out = pg.optimize(*args)
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out = pg.optimize(*args)
            ts.append(1e3 * (time.perf_counter() - t0))
        ctx.prof_enable(True)
        ctx.prof_reset()
        pg.optimize(*args)
        ctx.synchronize()
        rep = ctx.prof_report()
        ctx.prof_enable(False)
        phases = " ".join(f"{k.replace('pg_', '').replace('_kernel', '')} {v[1]:.2f}" for k, v in sorted(rep.items(), key=lambda kv: -kv[1][1]))
        g2o_ms, ratio = float("nan"), float("nan")
        if ref is not None:
            L = ref.build_driver()
            rs = []
            for _ in range(3):
                o = ref.solve(L, pr)
                rs.append(1e3 * float(o["seconds"][0]))
            g2o_ms = float(np.median(rs))
            ratio = g2o_ms / float(np.median(ts))
            if int(o["iters"][0]) != out["iterations"]:   # (the reference's step does not pin the count at every size: see DESIGN)
                print(f"note: g2o ran {int(o['iters'][0])} iterations, the device {out['iterations']}")
        lines.append(f"{n:9d} {pr['E']:5d} {7 * (n - 1):6d} {out['iterations']:5d} {int(out['trials'].sum()):6d} | {np.median(ts):8.2f} ({min(ts):.2f} .. {max(ts):.2f}) | "
                     f"{g2o_ms:10.2f} | {ratio:6.2f} | {phases}")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
