"""HIP-event timing of GlobalOptimizer.optimize() on problems with marker edges beside the marker-free wide form on the same landmarks.

  10 keyframes x 3000 landmarks (the bench's local-BA size) and 70 x 400, each with 0 / 2 / 4 markers seen by four frames.  The
  zero-marker leg runs through UH_BA_WIDE=1, so like is compared with like: a problem with marker edges always takes the wide form.
Events around optimize() on the optimiser's stream, REPS repetitions after WARM warm-up calls; median, 10th / 90th percentile, the
outer iterations and the launches per LM trial the wide form makes at that size.  Every problem is set in a
fresh child process, since the form switch is read from the environment.   python scripts/time_ba_markers.py [REPS]"""
import json
import os
import subprocess
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM = 5


def child(n_markers, K, P, reps):
    sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
    import numpy as np
    import torch

    import ba_marker_synth
    import ucoslam_cv3_amd as u
    from ucoslam_cv3_amd.ba import GlobalOptimizer, ParamSet

    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    ctx = u.Context(0, stream.cuda_stream)
    first = [1 + (K - 6) * i // max(n_markers - 1, 1) for i in range(n_markers)]
    pr = ba_marker_synth.marker_ba_problem(K=K, P=P, seed=0, stereo_frac=0.0, marker_frames=[list(range(f, f + 4)) for f in first] or [[0, 1]])
    markers = None
    if n_markers:
        markers = dict(pose_g2m=pr["mk_pose"], size=pr["mk_size"], edge_marker=pr["me_marker"], edge_frame=pr["me_frame"], und_corners=pr["me_corners"],
                       edge_weight=pr["me_weight"])
    opt = GlobalOptimizer.create(ctx)
    opt.setParams(pr, ParamSet(nIters=5), markers=markers)
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
    nfree = int((pr["fixed"] == 0).sum()) + n_markers
    panels = -(-6 * nfree // 64)
    launches = (9 if n_markers else 7) + 4 * panels - 1   # advance, two memsets, schur, assemble, (diag, panel, update, back) per panel, pose, backsub (+ marker assemble, marker lin)
    print(json.dumps(dict(markers=n_markers, edges=len(pr["me_marker"]) if n_markers else 0, K=K, P=pr["P"], E=pr["E"], form=opt.form(), iters=it, reps=reps,
                          launches_per_trial=launches, median_ms=round(float(np.median(ms)), 4), p10_ms=round(float(ms[len(ms) // 10]), 4),
                          p90_ms=round(float(ms[(9 * len(ms)) // 10]), 4), ms_per_iter=round(float(np.median(ms)) / max(sum(it), 1), 4))))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]))
        sys.exit(0)
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 60
    for K, P in ((10, 3000), (70, 400)):
        for n_markers in (0, 2, 4):
            env = {"UH_BA_WIDE": "1"} if n_markers == 0 else {}
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n_markers), str(K), str(P), str(reps)], env={**os.environ, **env},
                               capture_output=True, text=True, timeout=300)
            if r.returncode != 0:   # nothing more is started on the device after a failure
                sys.exit(f"{n_markers} markers {K}x{P} {env}: exit {r.returncode}\n{r.stdout}{r.stderr}")
            print((" ".join(f"{k}={v}" for k, v in env.items()) or "-").ljust(14), r.stdout.strip().splitlines()[-1], flush=True)
