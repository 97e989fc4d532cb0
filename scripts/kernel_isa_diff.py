#!/usr/bin/env python3
"""Compare the gfx950 code of every kernel in two builds of one source, without a GPU.

    kernel_isa_diff.py A.s B.s                  two device assembly files
    kernel_isa_diff.py TREE_A TREE_B ba.hip     two source trees: each csrc/<name> is compiled device-only with build.HIPCC_FLAGS

Per kernel: SAME / DIFF of the instruction stream (comments and directives stripped, .LBB labels renumbered), the instruction
count, whether the opcode histogram is equal, and the .amdhsa_* resource figures.  Exit status 1 on any DIFF and on a kernel
that only one side has.  --show N prints the first N differing lines of each DIFF kernel.
"""
import argparse, collections, importlib.util, os, re, subprocess, sys, tempfile

RES = {"next_free_vgpr": "vgpr", "next_free_sgpr": "sgpr", "accum_offset": "accum", "private_segment_fixed_size": "scratch",
       "group_segment_fixed_size": "lds", "kernarg_size": "kernarg"}


def compile_tree(tree, name, out):
    spec = importlib.util.spec_from_file_location("_uh_build", os.path.join(tree, "ucoslam-cv3_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    subprocess.run([b._hipcc(), *b.HIPCC_FLAGS, "--cuda-device-only", "-S", os.path.join(b.CSRC, name), "-o", out], check=True)
    return out


def parse(path):
    """{kernel symbol: (instruction lines, {resource: value})}"""
    text = open(path).read()
    kernels = {}
    for n in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M):
        q = re.escape(n)
        m = re.search(r"^%s:[^\n]*\n(.*?)^\s*\.amdhsa_kernel\s+%s\n(.*?)\.end_amdhsa_kernel" % (q, q), text, re.M | re.S)
        lines = [re.split(r";|//", l)[0].strip() for l in m.group(1).splitlines()]
        lines = [l for l in lines if l and (not l.startswith(".") or l.startswith(".LBB"))]
        labels = {}
        for l in lines:   # renumber the block labels in order of definition
            d = re.match(r"(\.LBB\w+):", l)
            if d:
                labels[d.group(1)] = ".L%d" % len(labels)
        ins = [re.sub(r"\.LBB\w+", lambda r: labels.get(r.group(0), r.group(0)), l) for l in lines if not l.endswith(":")]
        res = dict(re.findall(r"\.amdhsa_(\w+)\s+(\S+)", m.group(2)))
        kernels[n] = (ins, {short: res.get(k, "-") for k, short in RES.items()})
    return kernels


def compare(a, b, show=0, out=sys.stdout):
    """One line per kernel; returns how many kernels differ or exist on one side only."""
    bad = 0
    for n in sorted(set(a) | set(b)):
        if n not in a or n not in b:
            bad += 1
            print("ONLY-%s %s" % ("A" if n in a else "B", n), file=out)
            continue
        (ia, ra), (ib, rb) = a[n], b[n]
        same = ia == ib and ra == rb
        bad += not same
        hist = collections.Counter(l.split()[0] for l in ia) == collections.Counter(l.split()[0] for l in ib)
        count = len(ia) if len(ia) == len(ib) else "%d->%d" % (len(ia), len(ib))
        fig = " ".join("%s=%s" % (k, ra[k] if ra[k] == rb[k] else ra[k] + "->" + rb[k]) for k in ra)
        print("%s %s insns=%s hist=%s %s" % ("SAME" if same else "DIFF", n, count, "equal" if hist else "differs", fig), file=out)
        if not same:
            for i, x, y in [(i, x, y) for i, (x, y) in enumerate(zip(ia, ib)) if x != y][:show]:
                print("    @%d  A: %-56s B: %s" % (i, x, y), file=out)
    print("%d kernels, %d differ" % (len(set(a) | set(b)), bad), file=out)
    return bad


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("source", nargs="?", help="file name under csrc/, when a and b are source trees")
    ap.add_argument("--show", type=int, default=0, metavar="N")
    args = ap.parse_args(argv)
    with tempfile.TemporaryDirectory() as tmp:
        if args.source:
            args.a = compile_tree(args.a, args.source, os.path.join(tmp, "a.s"))
            args.b = compile_tree(args.b, args.source, os.path.join(tmp, "b.s"))
        return 1 if compare(parse(args.a), parse(args.b), args.show) else 0


if __name__ == "__main__":
    sys.exit(main())
