"""Time of the relocalisation pose search through the plugin boundary, two routes, at 1 and at 8 candidate keyframes:

  python scripts/time_relocalize.py [--calls 200] [--warmup 20] [--out FILE]

  (a) the composed chain through the C ABI, the calls of examples/relocalize.cpp: one uh_pnp_ransac for all candidates, then per survivor
      uh_projmatch_match, the host's id -> row look-ups and uh_pnp_solve.  The C structures are built once; inside the window are the
      calls and the look-ups between them (which a host cannot avoid).
  (b) uh_relocalize_pose: one call, one wait.

Workload (that of scripts/time_pnp_ransac.py): every candidate has 300 matches with 30 % gross outliers and 50 iterations, over a
2000-keypoint frame and 3000 points per candidate.  Reported: median / p10 / p90 of a host clock around a call that ends in its wait.
Per-kernel times come from a run of this script under `rocprofv3 --kernel-trace --stats` of its own."""
import argparse
import ctypes as C
import os
import sys
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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("time_relocalize.py needs a GPU: there is no CPU path to time")
    import synth
    import ucoslam_cv3_amd as u
    from ucoslam_cv3_amd import relocalize as R
    from ucoslam_cv3_amd._lib import lib, np_ptr
    from ucoslam_cv3_amd.orb import DeviceFrame
    from ucoslam_cv3_amd.pnp import PnPSolver
    from ucoslam_cv3_amd.projmatch import DMATCH_DTYPE, ProjectionMatcher, _MapPoints

    ctx = u.Context(0, None, private=True)
    fr, mp, pose_kf = synth.proj_problem(2000, 3000, seed=31)
    sf = fr["scale_factors"]
    inv_sf = (np.float32(1) / sf).astype(np.float32)
    intr = np.array([fr["fx"], fr["fy"], fr["cx"], fr["cy"]], np.float32)
    kps = fr["und_kpts"]
    mp = dict(mp, weight=np.ones(len(mp["ids"]), np.float32))
    pm_h, pnp_h = ProjectionMatcher(ctx), PnPSolver(ctx)
    rs = u.PnPRansac(pnp_h)
    pm_h.setFrame(kps, fr["desc"], sf, fr["fx"], fr["fy"], fr["cx"], fr["cy"], fr["min_xy"], fr["max_xy"])
    m0 = pm_h.matchFrameToMapPoints(pose_kf, mp["ids"], mp["pos3d"], mp["normal"], mp["min_dist"], mp["max_dist"], mp["desc"], 100.0, 15.0)["matches"]
    row = {int(v): i for i, v in enumerate(mp["ids"])}
    rows = np.array([row[int(t)] for t in m0["trainIdx"]], np.int64)
    dev = DeviceFrame(ctx).upload(kps, fr["desc"])
    pm_d, pnp_d = ProjectionMatcher(ctx), PnPSolver(ctx)
    pm_d.setFrameDev(dev, sf, fr["fx"], fr["fy"], fr["cx"], fr["cy"], fr["min_xy"], fr["max_xy"], und_kpts=kps)
    rt6 = R.se3_to_rt6(pose_kf)
    C.CDLL(None).srand(C.c_uint(1))
    lines = []
    for n_cand in (1, 8):
        cands = []
        for c in range(n_cand):
            rng = np.random.default_rng(900 + c)
            sel = rng.choice(len(m0), 300, replace=False)
            p3d, nrm = mp["pos3d"][rows[sel]].copy(), mp["normal"][rows[sel]].copy()
            out = rng.random(300) < 0.3   # gross outliers: another point's coordinates
            p3d[out], nrm[out] = np.roll(p3d[out], 7, axis=0), np.roll(nrm[out], 7, axis=0)
            cands.append(dict(matches=np.ascontiguousarray(m0[sel]), p3d=p3d, normal=nrm, rt6=rt6, points=mp, samples=u.ransac_samples(300, 50)))
        want = R.relocalize_pose(pm_h, pnp_h, rs, fr, cands, inv_sf, 50.0)
        got = R.relocalize_pose_onecall(pm_d, pnp_d, None, fr, cands, inv_sf, 50.0, n_keypoints=len(kps))
        assert want["best"] == got["best"] and want["n_matches"] == got["n_matches"] and [s["stage"] for s in want["steps"]] == [s["stage"] for s in got["steps"]]
        # ---- route (a): structures built once
        problems = [dict(p3d=k["p3d"], normal=k["normal"], kp=np.stack([kps["x"][k["matches"]["queryIdx"]], kps["y"][k["matches"]["queryIdx"]]], 1), samples=k["samples"], rt6_in=rt6)
                    for k in cands]
        call_r, ps, rr, bufs, keep = rs.prepare(intr, problems, want_counts=False)
        ids = np.ascontiguousarray(mp["ids"], np.uint32)
        arrs = [np.ascontiguousarray(mp[k], np.float32) for k in ("pos3d", "normal", "min_dist", "max_dist")] + [np.ascontiguousarray(mp["desc"], np.uint8)]
        mpp = _MapPoints(len(ids), np_ptr(ids), *[np_ptr(x) for x in arrs])
        mm = np.zeros(len(ids), DMATCH_DTYPE)
        pose_o, bad, iters = np.zeros(16, np.float32), np.zeros(len(ids), np.uint8), np.zeros(4, np.int32)
        id0 = int(ids.min())   # (the ids of synth.proj_problem are neither contiguous nor sorted: a table, as a host keeps one)
        table = np.full(int(ids.max()) + 1 - id0, -1, np.int64)
        table[ids.astype(np.int64) - id0] = np.arange(len(ids))
        L = lib()
        kx, ky, ko, pos, wgt = kps["x"], kps["y"], kps["octave"], arrs[0].reshape(-1, 3), mp["weight"]

        def route_a():
            assert call_r() == 0
            best, best_n = -1, 0
            for c in range(n_cand):
                r = rr[c]
                if (r.n_inliers if r.ok else 300) < 15:
                    continue
                pose = np.ctypeslib.as_array(r.pose)
                nm = L.uh_projmatch_match(pm_h._h, np_ptr(pose), C.byref(mpp), 100.0, 2.5, np_ptr(mm), len(mm), None, None, None)
                if nm < 30:
                    continue
                m = mm[:nm]
                rw, q = table[m["trainIdx"] - id0], m["queryIdx"]
                p3 = np.ascontiguousarray(pos[rw])
                kp = np.ascontiguousarray(np.stack([kx[q], ky[q]], 1))
                isg, w = np.ascontiguousarray(inv_sf[ko[q]]), np.ascontiguousarray(wgt[rw])
                L.uh_pnp_solve(pnp_h._h, np_ptr(pose), np_ptr(intr), nm, np_ptr(p3), np_ptr(kp), np_ptr(isg), np_ptr(w), np_ptr(pose_o), np_ptr(bad), np_ptr(iters), None)
                good = nm - int(np.count_nonzero(bad[:nm]))
                if good >= 30 and good > best_n:
                    best, best_n = c, good
            return best, best_n

        # ---- route (b): structures built once (the wrapper's, kept alive), nothing but the C call in the window
        isl = np.ascontiguousarray(inv_sf)
        args = R._RelocArgs(np_ptr(intr), np_ptr(isl), len(isl), 100.0, 2.5, 50, 25, 15, 30, 30)
        cs, ss = (R._RelocCandidate * n_cand)(), (R._RelocStep * n_cand)()
        hold = []
        for c, k in enumerate(cands):
            q = np.ascontiguousarray(k["matches"]["queryIdx"], np.int32)
            p3, nr, smp = np.ascontiguousarray(k["p3d"], np.float32), np.ascontiguousarray(k["normal"], np.float32), np.ascontiguousarray(k["samples"], np.int32)
            inl, mo, bo = np.zeros(300, np.int32), np.zeros(len(kps), DMATCH_DTYPE), np.zeros(len(kps), np.uint8)
            hold += [q, p3, nr, smp, inl, mo, bo]
            cs[c] = R._RelocCandidate(300, np_ptr(q), np_ptr(p3), np_ptr(nr), np_ptr(rt6), np_ptr(smp), C.pointer(mpp), np_ptr(wgt))
            ss[c].inliers, ss[c].cap_inliers, ss[c].matches_map, ss[c].bad, ss[c].cap_map = np_ptr(inl), 300, np_ptr(mo), np_ptr(bo), len(kps)
        res = R._RelocResult()
        res.steps = C.cast(ss, C.POINTER(R._RelocStep))
        csp = C.cast(cs, C.POINTER(R._RelocCandidate))

        def route_b():
            assert L.uh_relocalize_pose(pm_d._h, pnp_d._h, C.byref(args), n_cand, csp, C.byref(res)) == 0
            return res.best, res.n_matches

        ra, rb = route_a(), route_b()
        assert ra == rb == (want["best"], want["n_matches"]), (ra, rb, want["best"], want["n_matches"])
        ta, tb = [], []
        for i in range(a.warmup + a.calls):   # the two routes alternate so that drift hits both alike
            t0 = time.perf_counter(); route_a(); t1 = time.perf_counter(); route_b(); t2 = time.perf_counter()
            if i >= a.warmup:
                ta.append((t1 - t0) * 1e6); tb.append((t2 - t1) * 1e6)
        stages = [s["stage"] for s in want["steps"]]
        for name, t in (("(a) composed chain through the C ABI", ta), ("(b) uh_relocalize_pose", tb)):
            med, p10, p90 = pct(t)
            lines.append(f"{name}: {n_cand} candidate(s) x 300 matches x 50 iterations, 3000 points each: median {med:.1f} us  p10 {p10:.1f}  p90 {p90:.1f}  ({a.calls} calls)")
        lines.append(f"    winner {want['best']} with {want['n_matches']} good matches; solved candidates: {stages.count('solved')} of {n_cand}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
