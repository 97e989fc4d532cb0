#!/usr/bin/env python3
"""Times the mapper's fuse search (uh_fuse_search) and the whole search-and-fuse step.

  1. ONE search, 2000 keypoints x 1500 points and x 8000 points: the library call on prepared arguments (point table already in the
     handle, frame resident), median and spread over --reps calls after a warm-up.  The call is synchronous: it returns when the kernel's
     completion word has arrived.
  2. The same problem through uh_projmatch_match — projmatch.hip is the parent commit's file, untouched — on the same resident frame, the
     same points and an equal effective radius (maxRepjDist = 2.5, every normal towards the camera so that neither search widens).
     Expectation to check: fuse <= 1.25 x projmatch (same walk and drain; the margin covers the skip array and the third output array).
  3. The same search through uh_fuse_search_host on one core.  THIS IS THE LIBRARY'S OWN HOST FORM, NOT THE REFERENCE: the reference's
     function needs OpenCV and cannot be built here; nobody has measured it.
  4. The whole function for 20 neighbours (2000 keypoints each, 1500 points in the new keyframe) through the Python mirror, on the device and
     on the host form: total time and the share spent inside the 21 searches (the apply step between them is Python here, C++ in a host).

    python scripts/time_fuse.py [--out profiles/fuse_time.txt] [--reps 200]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
F = np.float32
W, H, FX, FY, CX, CY = 1241, 376, 718.856, 718.856, 607.19, 185.22
SCALE = np.cumprod(np.array([1] + [1.2] * 7, F)).astype(F)


def pose(rng, s):
    a = rng.normal(0, 0.02 * s, 3)
    Rx = np.array([[1, 0, 0], [0, np.cos(a[0]), -np.sin(a[0])], [0, np.sin(a[0]), np.cos(a[0])]])
    Ry = np.array([[np.cos(a[1]), 0, np.sin(a[1])], [0, 1, 0], [-np.sin(a[1]), 0, np.cos(a[1])]])
    T = np.eye(4)
    T[:3, :3] = Rx @ Ry
    T[:3, 3] = rng.normal(0, 0.3 * s, 3)
    return T.astype(F)


def project(T, X):
    c = X @ T[:3, :3].astype(np.float64).T + T[:3, 3]
    return np.stack([FX * c[:, 0] / c[:, 2] + CX, FY * c[:, 1] / c[:, 2] + CY], 1), c[:, 2]


def make_world(rng, n):
    return np.stack([rng.uniform(-9, 9, n), rng.uniform(-2.5, 2.5, n), rng.uniform(8, 14, n)], 1)


def make_keyframe(rng, idx, T, world, base, n_kpts):
    from oracle_lib import KEYPOINT_DTYPE

    uv, z = project(T, world)
    ok = np.nonzero((uv[:, 0] > 5) & (uv[:, 0] < W - 5) & (uv[:, 1] > 5) & (uv[:, 1] < H - 5) & (z > 1))[0]
    pick = rng.choice(ok, min(n_kpts, len(ok)), replace=False)
    k = np.zeros(len(pick), KEYPOINT_DTYPE)
    k["x"], k["y"] = (uv[pick] + rng.uniform(-0.3, 0.3, (len(pick), 2))).astype(F).T
    k["octave"] = rng.integers(1, 4, len(pick))
    desc = base[pick].copy()
    flips = rng.integers(0, 256, (len(pick), 6))
    for c in range(6):
        desc[np.arange(len(pick)), flips[:, c] >> 3] ^= (1 << (flips[:, c] & 7)).astype(np.uint8)
    return dict(idx=idx, pose_f2g=T, und_kpts=k, desc=desc, ids=np.full(len(pick), 0xFFFFFFFF, np.uint32), scale_factors=SCALE.copy(), fx=FX, fy=FY, cx=CX, cy=CY,
                min_xy=(0, 0), max_xy=(W, H), bad=False), pick


def make_points(rng, T, fr, n):
    """n points near keypoints of fr, normals towards the camera (viewCos ~ 1), levels matching the keypoints' octaves."""
    from fuse_oracle import camera_center

    k = fr["und_kpts"]
    j = rng.integers(0, len(k), n)
    z = rng.uniform(8, 14, n)
    uv = np.stack([k["x"][j], k["y"][j]], 1) + rng.uniform(-1.5, 1.5, (n, 2))
    xc = np.stack([(uv[:, 0] - CX) / FX * z, (uv[:, 1] - CY) / FY * z, z], 1)
    Td = T.astype(np.float64)
    pos = ((xc - Td[:3, 3]) @ Td[:3, :3]).astype(F)
    v = camera_center(T).astype(np.float64) - pos
    dist = np.linalg.norm(v, axis=1)
    maxd = (dist * 1.2 ** (k["octave"][j] + rng.uniform(-0.9, 0.4, n))).astype(F)
    desc = fr["desc"][j].copy()
    far = rng.random(n) < 0.3
    desc[far] = rng.integers(0, 256, (int(far.sum()), 32), dtype=np.uint8)
    return dict(ids=np.arange(n, dtype=np.uint32), pos3d=pos, normal=(v / dist[:, None]).astype(F), min_dist=(maxd / SCALE[-1]).astype(F), max_dist=maxd, desc=desc)


def stats(t):
    t = np.sort(np.array(t))
    return f"median {np.median(t):8.1f} us   p10 {t[len(t) // 10]:8.1f}   p90 {t[(9 * len(t)) // 10]:8.1f}   min {t[0]:8.1f}   (n = {len(t)})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    import torch

    import ucoslam_cv3_amd as u
    from ucoslam_cv3_amd import fuse as UF
    from ucoslam_cv3_amd._lib import check, lib, np_ptr
    from ucoslam_cv3_amd.orb import DeviceFrame
    from ucoslam_cv3_amd.projmatch import DMATCH_DTYPE, ProjectionMatcher, _MapPoints

    assert torch.cuda.is_available(), "needs a GPU: a time taken anywhere else says nothing"
    ctx = u.Context(0, torch.cuda.current_stream().cuda_stream)
    lines = ["fuse search timing (scripts/time_fuse.py): wall time of the synchronous library call on prepared arguments, microseconds", ""]
    rng = np.random.default_rng(99)
    world = make_world(rng, 6000)
    base = rng.integers(0, 256, (len(world), 32), dtype=np.uint8)
    T = pose(rng, 1)
    fr, _ = make_keyframe(rng, 1, T, world, base, 2000)
    dev = DeviceFrame(ctx).upload(fr["und_kpts"], fr["desc"])
    fs = UF.FuseSearch(ctx)
    pm = ProjectionMatcher(ctx)
    pm.setFrameDev(dev, fr["scale_factors"], FX, FY, CX, CY, (0, 0), (W, H))
    ratios = {}
    for n in (1500, 8000):
        pts = make_points(rng, T, fr, n)
        fs.setPoints(pts["pos3d"], pts["normal"], pts["min_dist"], pts["max_dist"], pts["desc"])
        f, keep = UF._frame_struct(fr, False)
        posef = np.ascontiguousarray(T, F).reshape(16)
        bk, bd, st = np.zeros(n, np.int32), np.zeros(n, F), np.zeros(n, np.uint8)
        call_fuse = lambda: check(lib().uh_fuse_search(fs._h, dev._h, C.byref(f), np_ptr(posef), np_ptr(SCALE), 8, None, 2.5, 1.4, 100.0, np_ptr(bk), np_ptr(bd), np_ptr(st)))   # noqa: E731
        mp = _MapPoints(n, *[np_ptr(pts[k]) for k in ("ids", "pos3d", "normal", "min_dist", "max_dist", "desc")])
        out = np.zeros(n, DMATCH_DTYPE)
        bk2, bd2, vis = np.zeros(n, np.int32), np.zeros(n, F), np.zeros(n, np.uint8)

        def call_pm():
            rc = lib().uh_projmatch_match(pm._h, np_ptr(posef), C.byref(mp), 100.0, 2.5, np_ptr(out), n, np_ptr(bk2), np_ptr(bd2), np_ptr(vis))
            assert rc >= 0

        for _ in range(20):
            call_fuse(); call_pm()
        tf, tp = [], []
        for _ in range(a.reps):   # alternating: both see the same machine
            t0 = time.perf_counter(); call_fuse(); t1 = time.perf_counter(); call_pm(); t2 = time.perf_counter()
            tf.append(1e6 * (t1 - t0)); tp.append(1e6 * (t2 - t1))
        host = UF.search_host(pts, fr, T, SCALE, None, 2.5, 1.4, 100.0)
        assert np.array_equal(host["best_kp"], bk) and np.array_equal(host["status"], st) and host["best_dist"].tobytes() == bd.tobytes(), "device form != host form"
        th = []
        for _ in range(max(5, a.reps // 20)):
            t0 = time.perf_counter(); UF.search_host(pts, fr, T, SCALE, None, 2.5, 1.4, 100.0); th.append(1e6 * (time.perf_counter() - t0))
        hist = np.bincount(st, minlength=6).tolist()
        ratios[n] = float(np.median(tf) / np.median(tp))
        lines += [f"one search, 2000 keypoints x {n} points (status histogram {hist}; projmatch visible {int(vis.sum())}, matched {int((bk2 >= 0).sum())}; fuse found {hist[0]})",
                  f"  uh_fuse_search                              {stats(tf)}",
                  f"  uh_projmatch_match (parent's file, r = 2.5) {stats(tp)}",
                  f"  ratio of the medians fuse / projmatch       {ratios[n]:.3f}   (expectation: <= 1.25)",
                  f"  uh_fuse_search_host, one core               {stats(th)}   <- the library's own host form incl. its kd-tree build, NOT the reference",
                  f"  device form against the host form           {np.median(th) / np.median(tf):.1f} x faster; outputs equal bit for bit", ""]
        del keep

    # ---- the whole function: 20 neighbours
    rng = np.random.default_rng(100)
    kfs, picks = {}, {}
    cur_idx = 100
    for i in [cur_idx] + list(range(20)):
        kfs[i], picks[i] = make_keyframe(rng, i, pose(rng, 1 if i != cur_idx else 0.2), world, base, 2000)
    m = dict(keyframes=kfs, map_points={}, neighbors={cur_idx: list(range(20))})
    nid = 0
    for i, kf in kfs.items():   # 1500 points in the new keyframe, 600 in each neighbour, each observed where it was made
        for kp in rng.choice(len(kf["ids"]), 1500 if i == cur_idx else 600, replace=False):
            w = world[picks[i][kp]]
            m["map_points"][nid] = dict(id=nid, pos3d=(w + rng.normal(0, 0.01, 3)).astype(F), normal=np.zeros(3, F), min_dist=F(0), max_dist=F(0), desc=np.zeros(32, np.uint8),
                                        frames={i: int(kp)}, bad=False)
            kf["ids"][kp] = nid
            nid += 1
    for pid in m["map_points"]:
        UF.updatePointInfo(m, pid)
    import copy

    frames = {i: DeviceFrame(ctx).upload(kf["und_kpts"], kf["desc"]) for i, kf in kfs.items()}
    clock = dict(t=0.0, n=0)

    def timed(fn):
        def g(*x, **kw):
            t0 = time.perf_counter()
            r = fn(*x, **kw)
            clock["t"] += time.perf_counter() - t0
            clock["n"] += 1
            return r
        return g

    real_dev, real_host = UF.FuseSearch.search, UF.search_host
    UF.FuseSearch.search, UF.search_host = timed(real_dev), timed(real_host)
    res = {}
    for form in ("device", "host", "device", "host"):
        mm = copy.deepcopy(m)
        clock.update(t=0.0, n=0)
        t0 = time.perf_counter()
        removed = UF.search_in_neighbors(mm, cur_idx, 100.0, fuser=fs if form == "device" else None, dev_frames=frames)
        total = time.perf_counter() - t0
        res.setdefault(form, []).append((total, clock["t"], clock["n"], len(removed), sum(len(p["frames"]) for p in mm["map_points"].values())))
    UF.FuseSearch.search, UF.search_host = real_dev, real_host
    lines.append("whole function, 20 neighbours x 2000 keypoints, 1500 points in the new keyframe, 600 in each neighbour (Python mirror; second of two runs):")
    for form in ("device", "host"):
        total, ts, ns, nrem, nobs = res[form][-1]
        lines.append(f"  {form:6s} form: {ns} searches {1e3 * ts:9.2f} ms (incl. the mirror's packing of each call), whole call {1e3 * total:9.2f} ms; {nrem} points fused away, {nobs} observations")
    assert res["device"][-1][3:] == res["host"][-1][3:]
    lines.append(f"  searches: host form / device form = {res['host'][-1][1] / res['device'][-1][1]:.1f}   (the host leg is the library's own host form on one core, NOT the reference)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(text + "\n")


if __name__ == "__main__":
    main()
