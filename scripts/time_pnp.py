#!/usr/bin/env python
"""Pose-only solve (uh_pnp_solve, host in / host out): wall time per call and the kernel's own clock stamps, by match count.
--stereo: uh_pnp_solve_stereo on tests/stereo_synth.py problems (about 60 % of the matches with a depth); --n N1,N2,..: the match counts;
--markers M1,M2,..: every match count also with that many markers (tests/marker_synth.py; 0 = the marker-free call, uh_pnp_solve_markers
with one or more); --reps R: the wall time R times over (the spread of a number measured against another build); --dump FILE: pose,
state, bad, iters and ngood of one solve per configuration into FILE (.npz), to compare two builds byte for byte."""
import sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import synth
import stereo_synth
import marker_synth
import ucoslam_cv3_amd as u
from ucoslam_cv3_amd.pnp import PnPSolver

ctx = u.Context(0, private=True)
sol = PnPSolver(ctx)
stereo = "--stereo" in sys.argv
counts = (100, 300, 600, 800, 1300, 1500, 3000, 4000)
if "--n" in sys.argv:
    counts = tuple(int(v) for v in sys.argv[sys.argv.index("--n") + 1].split(","))
marker_counts = (0,)
if "--markers" in sys.argv:
    marker_counts = tuple(int(v) for v in sys.argv[sys.argv.index("--markers") + 1].split(","))
reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 1
dump, dumped = (sys.argv[sys.argv.index("--dump") + 1] if "--dump" in sys.argv else None), {}
for n, n_mk in ((n, m) for n in counts for m in marker_counts):
    pr = stereo_synth.stereo_pnp_problem(n, seed=3) if stereo else synth.pnp_problem(n, seed=3)
    args = (pr["pose"], pr["intr"], pr["p3d"], pr["kp"], pr["invsig"], pr["weight"])
    kw = dict(depth=pr["depth"], bl=pr["bl"]) if stereo else {}
    if n_mk:
        kw["markers"] = marker_synth.make_markers(np.random.default_rng(3), pr["pose_gt"], pr["intr"], n_mk)
    for _ in range(5):
        r = sol.solvePnp(*args, **kw)
    walls = []
    for _ in range(reps):
        t = time.perf_counter()
        for _ in range(50):
            r = sol.solvePnp(*args, **kw)
        walls.append((time.perf_counter() - t) / 50 * 1e6)
    wall = walls[-1]
    for k in ("pose", "state", "bad", "iters", "ngood") if dump else ():
        dumped[f"{'stereo' if stereo else 'mono'}_n{n}_mk{n_mk}_{k}"] = np.asarray(r[k])
    sol.debug_clocks(True)
    sol.solvePnp(*args, **kw)
    c = sol.debug_clocks(True)
    if os.environ.get("PNP_TRACE"):
        sol.debug_clocks(True); sol.solvePnp(*args, **kw); c = sol.debug_clocks(True)
        tr = c[8:8 + int(c[4]) + 2]
        print("   trials (round.it:qmax+/-):", " ".join(f"{(v >> 16) & 255}.{(v >> 8) & 255}:{v & 255}{'+' if v >> 24 else '-'}" for v in tr if v))
    sol.debug_clocks(False)
    tot = c[3] - c[0]
    print("   wave 0 cycles: prepare(solve+update) %d  barrierA %d  matches+butterfly %d  barrierB %d  totals+decision %d  ladder passes %d" % tuple(c[16:22]))
    if reps > 1:
        print("   wall per call over the repetitions [us]:", " ".join(f"{w:.1f}" for w in walls))
    print(f"{'stereo ' if stereo else ''}{f'markers {n_mk} ' if n_mk else ''}n={n:5d} wall {wall:7.1f} us  iters {r['iters'].tolist()} passes {c[4]}  clk: stage {c[1]-c[0]} rounds {c[2]-c[1]} post {c[3]-c[2]} total {tot}  per pass {(c[2]-c[1])/max(c[4],1):.0f}")
if dump:
    np.savez(dump, **dumped)
