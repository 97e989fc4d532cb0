"""Time of uh_pnp_ransac (the relocalisation RANSAC) through the plugin boundary: host arrays in, results out, one wait per call.

  python scripts/time_pnp_ransac.py [--calls 200] [--warmup 20] [--no-host] [--out FILE]

Shapes: 1 and 8 candidate keyframes x 300 matches x 50 iterations (30 % gross outliers), what System::relocalize hands the function.
Reported: median / p10 / p90 of the wall time of a call (a host clock around a call that ends in a stream synchronise) — of the C entry
alone on prebuilt structures, for both forms of the hypothesis kernel (uh_pnp_ransac_debug_form) alternating call by call, and of the
Python mirror, which packs the problems inside the window.  The comparison
point is the HOST BUILD OF THE SAME ARITHMETIC (csrc/p3p_math.hpp through tests/host_helpers/p3p_math_host.cpp, g++ -O2, one core, the
candidates one after the other): the reference's own function cannot be built without OpenCV, so this is NOT the reference's time.
Per-kernel times come from a run of this script under `rocprofv3 --kernel-trace --stats` of its own (with --no-host)."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def pct(x):
    x = np.sort(np.asarray(x))
    return float(np.median(x)), float(x[int(0.1 * (len(x) - 1))]), float(x[int(0.9 * (len(x) - 1))])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("time_pnp_ransac.py needs a GPU: there is no CPU path to time")
    import pnp_ransac_synth as S
    import ucoslam_cv3_amd as u

    ctx = u.Context(0, None, private=True)
    rs = u.PnPRansac(ctx)
    lines = []
    host = None
    if not a.no_host:
        so = os.path.join(tempfile.mkdtemp(), "libp3p_math_host.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                               os.path.join(ROOT, "tests", "host_helpers", "p3p_math_host.cpp")])
        host = C.CDLL(so)
    P = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731
    def timed(fn, calls):
        t = []
        for _ in range(calls):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e6)
        return pct(t)

    for cands in (1, 8):
        prs = [S.scene(900 + c, 300, 50, outliers=0.3) for c in range(cands)]
        # (1) the C entry alone: the structures are built once, the timed window holds nothing but uh_pnp_ransac (its checks, packing, upload,
        # two launches, download, wait); the two forms of the hypothesis kernel alternate call by call so that drift hits both alike
        call, ps, results, bufs, keep = rs.prepare(S.INTR, prs, want_counts=False)
        forms = {False: [], True: []}
        for i in range(2 * (a.warmup + a.calls)):
            uniform = bool(i & 1)
            rs.set_form(uniform)
            t0 = time.perf_counter()
            rc = call()
            dt = (time.perf_counter() - t0) * 1e6
            if rc != 0:
                sys.exit(f"uh_pnp_ransac failed: {rc}")
            if i >= 2 * a.warmup:
                forms[uniform].append(dt)
        rs.set_form(False)
        for uniform, name in ((False, "one root per lane (built)"), (True, "all four roots on every lane")):
            med, p10, p90 = pct(forms[uniform])
            lines.append(f"uh_pnp_ransac, C entry alone, {name}: {cands} candidate(s) x 300 matches x 50 iterations: median {med:.1f} us  p10 {p10:.1f}  "
                         f"p90 {p90:.1f}  ({a.calls} calls)")
        # (2) through the Python mirror, which packs the problems inside the window
        for _ in range(a.warmup):
            res = rs.solve(S.INTR, prs, want_counts=False)
        med, p10, p90 = timed(lambda: rs.solve(S.INTR, prs, want_counts=False), a.calls)
        res = rs.solve(S.INTR, prs, want_counts=False)
        lines.append(f"PnPRansac.solve (Python mirror, packing included): {cands} candidate(s): median {med:.1f} us  p10 {p10:.1f}  p90 {p90:.1f}  "
                     f"({a.calls} calls; inliers {[r['n_inliers'] for r in res]})")
        if host is not None:
            best = []

            def host_all():
                best.clear()
                for pr in prs:
                    counts, rt6 = np.zeros(50, np.int32), np.zeros(6, np.float32)
                    best.append(host.p3p_host_ransac(P(pr["intr"]), pr["n"], P(pr["p3d"]), P(pr["normal"]), P(pr["kp"]), 50, P(pr["samples"]), P(counts), P(rt6)))

            med, p10, p90 = timed(host_all, max(a.calls // 4, 10))
            lines.append(f"host build of the same arithmetic, one core, {cands} candidate(s): median {med:.1f} us  p10 {p10:.1f}  p90 {p90:.1f}  "
                         f"(winners {best} against the device's {[r['best_iter'] for r in res]})")
    rs.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
