#!/usr/bin/env python
"""Which kernels the exact search launches for which call: a fixed list of searches around every threshold of the form decision
(knn.hip: plan_search), to be compared between two builds of the library.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python scripts/knn_launch_trace.py run > run.log
    python scripts/knn_launch_trace.py compare A_kernel_trace.csv B_kernel_trace.csv [A_run.log B_run.log] [--out LIST]

run      performs the searches in one process and prints, per case, the profiler scope names of its launches (Context.prof_report) and
         a checksum of a search's rows (results are not checked against an oracle: that is the tests' job).
compare  diffs, in launch order, the knn_* rows of two kernel traces — kernel with template arguments, grid, workgroup and LDS size —
         and the scope lines of the two run logs; exit status 1 on any difference.  --out writes side B's list (launches, then scopes).
"""
import argparse, csv, difflib, os, re, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run():
    sys.path.insert(0, ROOT)
    import numpy as np, torch
    import ucoslam_cv3_amd as u
    from ucoslam_cv3_amd.knn import Index, shard_bounds

    torch.cuda.set_device(0)
    ctx = u.Context(0, torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(0)
    train = rng.integers(0, 256, (10000, 32), dtype=np.uint8)
    d_train = torch.from_numpy(train).cuda()
    d_q = torch.from_numpy(rng.integers(0, 256, (32769, 32), dtype=np.uint8)).cuda()
    knobs = ("UH_KNN_FORM", "UH_KNN_ACCEPT_QPW", "UH_KNN_SHARD_FORM")

    def index(rows=10000, ctx=ctx, **env):   # the knobs are read when an index is created (UH_KNN_SHARD_FORM: or per call) — they stay set until the next index
        for k in knobs:
            os.environ.pop(k, None)
        os.environ.update(env)
        return Index(ctx).build(d_train[:rows])

    def case(label, fn, ctx=ctx):
        ctx.prof_enable(True); ctx.prof_reset()
        out = fn()
        torch.cuda.synchronize()
        names = sorted(k for k, v in ctx.prof_report().items() if v[0])
        ctx.prof_enable(False)
        rows = " rows %d" % (int(out[0].sum().item()) ^ int(out[1].sum().item())) if out else ""
        print("scopes %s: %s%s" % (label, " | ".join(names), rows), flush=True)

    def searches(tag, idx, nqs, nns, ctx=ctx):
        for nq in nqs:
            for nn in nns:
                case("%s nq=%d nn=%d" % (tag, nq, nn), lambda: idx.search(d_q[:nq], nn), ctx)

    searches("rows=10000", index(), (1, 64, 2016, 2017, 3024, 3025, 4032, 4033, 8000, 32768, 32769), (1, 2, 3, 4, 5, 6, 10, 15, 16, 17, 64))
    for rows in (300, 40):   # the capacity clamp keeps the stream form out
        searches("rows=%d" % rows, index(rows), (64, 2500), (2, 10))
    for form in ("fused", "twophase", "stream", "split"):
        searches("form=" + form, index(UH_KNN_FORM=form), (100, 2000, 5000), (2, 10, 17))
    for qpw in (2, 4):
        searches("form=fused qpw=%d" % qpw, index(UH_KNN_FORM="fused").set_queries_per_wave(qpw), (2000,), (3, 4, 15, 16))
    searches("accept_qpw=1", index(UH_KNN_ACCEPT_QPW="1"), (8000,), (2, 10))
    # a context on 32 compute units: the thresholds scale with them, so that nn <= 5 reaches the fused form and UH_KNN_FORM=split its own
    # (its stream is its own: every case ends in a device-wide synchronise before the rows are read)
    few_cus = u.Context(0, cus=(0, 32))
    for env in ({}, {"UH_KNN_FORM": "split"}):
        searches("cus=32 form=%s" % env.get("UH_KNN_FORM", "default"), index(ctx=few_cus, **env), (300, 700, 2000, 5000), (2, 5, 10), few_cus)

    # the shard API: every tile's scan (an index of its own with a row offset), then both replays of the gathered lists
    nq = 2000
    for form in (None, "lanes", "old"):
        env = {"UH_KNN_SHARD_FORM": form} if form else {}
        for world in (1, 8):
            b = shard_bounds(len(train), world)
            whole = index(**env)
            tiles = [Index(ctx).build(d_train[b[s]:b[s + 1]].contiguous()).set_row_offset(b[s]) for s in range(world)]
            for nn in (2, 10, 17):
                for cap in (32, 256, 512):
                    def shard_case():
                        lists = [t.scan_shard(d_q[:nq], nn, cap) for t in tiles]
                        cand, cnt = torch.stack([c for c, _ in lists]), torch.stack([n for _, n in lists])
                        whole.replay(d_q[:nq], nn, cand, cnt)
                        tiles[0].replay_tiles(d_q[:nq], nn, cand, cnt)
                    case("shards form=%s world=%d nn=%d cap=%d" % (form or "unset", world, nn, cap), shard_case)


def launches(path, prefix="knn_"):
    """One line per dispatch of a rocprofv3 kernel trace whose kernel name begins with `prefix`, in dispatch order."""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Dispatch_Id"]))
    def dims(r, what):
        return "x".join(r[k] for k in (what + "_X", what + "_Y", what + "_Z")) if what + "_X" in r else r[what]
    out = []
    for r in rows:
        m = re.search(prefix + r"\w+(<[^>]*>)?", r["Kernel_Name"])
        if m:
            out.append("%s grid %s block %s lds %s" % (m.group(0), dims(r, "Grid_Size"), dims(r, "Workgroup_Size"), r["LDS_Block_Size"]))
    return out


def scopes(path):
    return [l.rstrip("\n") for l in open(path) if l.startswith("scopes ")]


def compare(args, prefix="knn_"):   # (scripts/ba_launch_trace.py: prefix "ba_")
    a, b = launches(args.a, prefix), launches(args.b, prefix)
    if args.log_a and args.log_b:
        a += scopes(args.log_a); b += scopes(args.log_b)
    if args.out:
        open(args.out, "w").write("\n".join(b) + "\n")
    diff = list(difflib.unified_diff(a, b, args.a, args.b, lineterm="", n=1))
    print("\n".join(diff) if diff else "%d lines on both sides, no difference" % len(a))
    return 1 if diff or not a else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="mode", required=True)
    sub.add_parser("run")
    c = sub.add_parser("compare")
    c.add_argument("a"); c.add_argument("b"); c.add_argument("log_a", nargs="?"); c.add_argument("log_b", nargs="?"); c.add_argument("--out")
    args = ap.parse_args()
    sys.exit(run() if args.mode == "run" else compare(args))
