#!/usr/bin/env python
"""Which kernels bundle adjustment launches for which problem: a fixed list of windows on both sides of every threshold of the
plan (ba.hip: plan_ba), to be compared between two builds of the library.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python scripts/ba_launch_trace.py run [--root TREE] > run.log
    python scripts/ba_launch_trace.py run --timed [--root TREE] > timed.log
    python scripts/ba_launch_trace.py compare A_kernel_trace.csv B_kernel_trace.csv [A_run.log B_run.log] [--out LIST]

run      setParams + optimize + getResults once per case in one process; prints, per case, the form, the profiler scope names of its
         launches (Context.prof_report) and a SHA-256 of every result array (results are not checked against an oracle: that is
         the tests' job).  --timed: the sizes bench.py times instead of the threshold windows.  --root: the tree whose library runs.
compare  knn_launch_trace.py's, on the ba_* rows of two kernel traces and the scope lines of the two run logs.
"""
import argparse, hashlib, os, sys

HERE = os.path.dirname(os.path.abspath(__file__))
KNOBS = ("FORM", "WIDE", "NF", "LW", "NSPLIT", "SOLVE", "PREBUILT", "SCHUR_DENSE", "DENSE_G", "SPEC", "OBS24", "NO_AVX512", "FAIL_RESIDENCY")


def run(root, timed):
    sys.path[:0] = [root, os.path.join(root, "tests")]
    import torch
    import ucoslam_cv3_amd as u
    from ucoslam_cv3_amd.ba import GlobalOptimizer, ParamSet
    import synth, het_ba_synth as het

    torch.cuda.set_device(0)
    ctx = u.Context(0, torch.cuda.current_stream().cuda_stream)
    shared = GlobalOptimizer(ctx)

    def case(label, pr, go=shared, stereo=None, staged=False, iters=5, late_env=None, **env):
        for k in KNOBS:
            os.environ.pop("UH_BA_" + k, None)
        os.environ.update({"UH_BA_" + k: v for k, v in env.items()})
        ctx.prof_enable(True); ctx.prof_reset()
        if staged:
            go.setParamsStaged(*go.fillStaging(pr), ParamSet(nIters=iters))
        else:
            go.setParams(pr, ParamSet(nIters=iters), stereo=stereo)
        planned = go.form()
        os.environ.update(late_env or {})
        go.optimize()
        out = go.getResults()
        torch.cuda.synchronize()
        names = sorted(k for k, v in ctx.prof_report().items() if v[0])
        ctx.prof_enable(False)
        sha = " ".join("%s=%s" % (k, hashlib.sha256(out[k].tobytes()).hexdigest()[:16]) for k in ("poses", "points", "chi2", "bad", "iters", "state"))
        print("scopes %s: %s->%s | %s | %s" % (label, planned, go.form(), " | ".join(names), sha), flush=True)

    def mono(nfree, P=200):
        return synth.ba_problem(nfree + 2, P, seed=nfree, nfixed=2)

    if timed:
        case("10x3000", synth.ba_problem(10, 3000, seed=0))
        for nfree in (17, 32, 48, 64):
            case("free=%d x3000" % nfree, mono(nfree, 3000))
        case("global 100x5000", synth.ba_problem(100, 5000, seed=1, nfixed=2), iters=10)
        case("stereo " + het.BENCH_CASE[0], het.het_ba_problem(**het.BENCH_CASE[1]), stereo=True)
        return 0
    for nfree in (1, 8, 9, 16, 17, 21, 22, 32, 33, 40, 48, 64, 65):
        case("mono free=%d" % nfree, mono(nfree))
    for name in ("het8", "het18", "het19", "het35", "het67"):   # 6, 16, 17, 33, 65 free keyframes
        case("stereo " + name, het.het_ba_problem(**het.CASES[name]), stereo=True)
    for env, windows in ((dict(FORM="legacy"), (8, 16)), (dict(NF="16"), (6,)), (dict(WIDE="1"), (6,)), (dict(SCHUR_DENSE="0"), (17, 24, 48)),
                         (dict(PREBUILT="0"), (17, 40)), (dict(SOLVE="hbm", FORM="legacy"), (8,)), (dict(SOLVE="hbm"), (32,)),
                         (dict(NSPLIT="3", FORM="legacy"), (12,))):
        for nfree in windows:
            case("mono free=%d %s" % (nfree, " ".join("%s=%s" % kv for kv in sorted(env.items()))), mono(nfree), **env)
    case("staged free=8", mono(8), staged=True)
    case("staged free=20", mono(20), staged=True)
    case("fail_residency free=8", mono(8), go=GlobalOptimizer(ctx), late_env={"UH_BA_FAIL_RESIDENCY": "1"})
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="mode", required=True)
    r = sub.add_parser("run")
    r.add_argument("--root", default=os.path.dirname(HERE)); r.add_argument("--timed", action="store_true")
    c = sub.add_parser("compare")
    c.add_argument("a"); c.add_argument("b"); c.add_argument("log_a", nargs="?"); c.add_argument("log_b", nargs="?"); c.add_argument("--out")
    args = ap.parse_args()
    if args.mode == "run":
        sys.exit(run(os.path.abspath(args.root), args.timed))
    sys.path.insert(0, HERE)
    import knn_launch_trace
    sys.exit(knn_launch_trace.compare(args, prefix="ba_"))
