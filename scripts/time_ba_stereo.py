"""HIP-event timing of GlobalOptimizer.optimize() with stereo / RGB-D observations beside the monocular forms on the same geometry.

  mono / mix (60 % of the observations with depth) / rgbd (all) on 10 keyframes x 3000 landmarks (the bench's local-BA size) in the
  launch chain (the monocular one under UH_BA_FORM=legacy), the monocular persistent form for the record, and 70 x 400 in the wide form.
Events around optimize() on the optimiser's stream, REPS repetitions after WARM warm-up calls; median, 10th / 90th percentile and the
outer iterations (a stereo problem may take other LM steps than the monocular one: compare per iteration as well).
Every problem is set in a fresh child process, since the form switches are read from the environment.   python scripts/time_ba_stereo.py [REPS]"""
import json
import os
import subprocess
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM = 5


def child(kind, K, P, reps):
    sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
    import numpy as np
    import torch

    import stereo_ba_synth
    import ucoslam_cv3_amd as u
    from ucoslam_cv3_amd.ba import GlobalOptimizer, ParamSet

    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    ctx = u.Context(0, stream.cuda_stream)
    frac = {"mono": 0.0, "mix": 0.6, "rgbd": 1.0}[kind]
    pr = stereo_ba_synth.stereo_ba_problem(K=K, P=P, seed=0, stereo_frac=frac)
    opt = GlobalOptimizer.create(ctx)
    opt.setParams(pr, ParamSet(nIters=5), stereo=True if frac > 0 else None)
    for _ in range(WARM):
        opt.optimize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        opt.optimize()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    it = opt.getResults()["iters"].tolist()
    ms = np.sort(np.array(ms))
    print(json.dumps(dict(kind=kind, K=K, P=pr["P"], E=pr["E"], stereo=int((pr["obs_depth"] > 0).sum()), form=opt.form(), iters=it, reps=reps,
                          median_ms=round(float(np.median(ms)), 4), p10_ms=round(float(ms[len(ms) // 10]), 4), p90_ms=round(float(ms[(9 * len(ms)) // 10]), 4),
                          ms_per_iter=round(float(np.median(ms)) / max(sum(it), 1), 4))))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]))
        sys.exit(0)
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    runs = [("mono", 10, 3000, {"UH_BA_FORM": "legacy"}), ("mix", 10, 3000, {}), ("rgbd", 10, 3000, {}), ("mono", 10, 3000, {}),
            ("mono", 70, 400, {}), ("mix", 70, 400, {})]
    for kind, K, P, env in runs:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, str(K), str(P), str(reps)], env={**os.environ, **env},
                           capture_output=True, text=True, timeout=300)
        if r.returncode != 0:   # nothing more is started on the device after a failure
            sys.exit(f"{kind} {K}x{P} {env}: exit {r.returncode}\n{r.stdout}{r.stderr}")
        print((" ".join(f"{k}={v}" for k, v in env.items()) or "-").ljust(20), r.stdout.strip().splitlines()[-1], flush=True)
