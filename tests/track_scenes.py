"""Tracker scenes held the way the reference holds its map (one table of map points keyed by id; the previous frame's items and the local
map name ids in it), for oracle_track_pose (tests/oracle_lib.py track_pose) and the inputs uh_track_pose takes, derived from the same
table.  Geometry as tests/test_track.py::_scene: map points behind the frame's keypoints, seen from a slightly different pose."""
import numpy as np

W, H = 1241, 376
FX, FY, CX, CY = 718.856, 718.856, 607.19, 185.22
SF = np.cumprod(np.concatenate([[np.float32(1)], np.full(7, np.float32(1.2))]).astype(np.float32)).astype(np.float32)
INV_SF = (np.float32(1) / SF).astype(np.float32)
INTR = np.array([FX, FY, CX, CY], np.float32)
ANISO = (655.1, 742.3, 633.7, 171.4)   # an anisotropic camera with its principal point elsewhere (fx, fy, cx, cy), for the intr= arguments
BL = 0.54
_A = 0.01
R0 = np.array([[np.cos(_A), 0, np.sin(_A)], [0, 1, 0], [-np.sin(_A), 0, np.cos(_A)]])
T0 = np.array([0.3, -0.05, 0.1])


def _camera(intr):
    return (FX, FY, CX, CY) if intr is None else tuple(float(v) for v in intr)


def frame(ukp, desc, intr=None):
    """The oracle's frame dict (synth.proj_problem's layout) for undistorted keypoints ukp (KEYPOINT_DTYPE) and their descriptors.
    intr=(fx, fy, cx, cy) replaces the module's camera."""
    fx, fy, cx, cy = _camera(intr)
    return dict(und_kpts=np.ascontiguousarray(ukp), desc=np.ascontiguousarray(desc, np.uint8).reshape(-1, 32), scale_factors=SF, fx=fx, fy=fy, cx=cx, cy=cy,
                min_xy=(0, 0), max_xy=(W, H))


def scene(ukp, desc, seed, n_prev=800, n_map=3000, pose_noise=0.0, in_map=0.7, unstable=0.2, stable_outside=False, uv_noise=0.7, intr=None):
    """n_map local-map points (ids 10...) and n_prev previous-frame items, a fraction `in_map` of them local-map points themselves (same
    id, hence the same position and stability), the others points of the table outside the local map (ids 100000...: a copy of a local
    point's geometry and descriptor under an id of their own).  unstable: the fraction of non-stable points (weight 0.5);
    stable_outside: every point outside the local map is stable (uh_track_pose has no weight input for those).
    intr=(fx, fy, cx, cy) replaces the module's camera; the scene carries its camera as "intr" (float32[4])."""
    FX, FY, CX, CY = _camera(intr)
    rng = np.random.default_rng(seed)
    n_k = len(ukp)
    und = np.stack([ukp["x"], ukp["y"]], 1).astype(np.float64)
    pick = rng.integers(0, max(n_k, 1), n_map)
    z = rng.uniform(4, 40, n_map)
    uv = (und[pick] if n_k else np.zeros((n_map, 2))) + rng.normal(0, uv_noise, (n_map, 2))
    Xc = np.stack([(uv[:, 0] - CX) / FX * z, (uv[:, 1] - CY) / FY * z, z], 1)
    Xw = (Xc - T0) @ R0
    cc = -R0.T @ T0
    view = cc - Xw
    dist = np.linalg.norm(view, axis=1)
    nrm = view / dist[:, None] + rng.normal(0, 0.3, (n_map, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    octs = ukp["octave"][pick] if n_k else np.zeros(n_map, np.int32)
    lev = np.clip(octs + rng.integers(-1, 2, n_map), 0, 7)
    maxd = dist * SF[lev] * rng.uniform(0.93, 1.07, n_map)
    kd = desc[pick] if n_k else np.zeros((n_map, 32), np.uint8)
    mdesc = kd ^ np.packbits(rng.random((n_map, 256)) < 0.04, axis=1, bitorder="little")
    local = dict(ids=np.arange(10, 10 + n_map, dtype=np.uint32), pos3d=Xw.astype(np.float32), normal=nrm.astype(np.float32),
                 min_dist=(maxd / SF[7]).astype(np.float32), max_dist=maxd.astype(np.float32), desc=np.ascontiguousarray(mdesc),
                 stable=(rng.random(n_map) >= unstable).astype(np.uint8))
    rows = np.sort(rng.choice(n_map, n_prev, replace=False)) if n_prev else np.zeros(0, np.int64)
    inm = rng.random(n_prev) < in_map
    out_rows = rows[~inm]
    n_out = len(out_rows)
    out_ids = (100000 + np.arange(n_prev, dtype=np.uint32))[~inm]
    out_stable = np.ones(n_out, np.uint8) if stable_outside else (rng.random(n_out) >= 0.4).astype(np.uint8)
    table = {k: np.concatenate([local[k], local[k][out_rows]]) for k in ("pos3d", "normal", "min_dist", "max_dist", "desc")}
    table["ids"] = np.concatenate([local["ids"], out_ids]).astype(np.uint32)
    table["stable"] = np.concatenate([local["stable"], out_stable]).astype(np.uint8)
    prev_ids = np.where(inm, local["ids"][rows] if n_prev else np.zeros(0, np.uint32), 100000 + np.arange(n_prev)).astype(np.uint32)
    prev = dict(ids=prev_ids, octave=octs[rows].astype(np.int32), desc=np.ascontiguousarray(local["desc"][rows]))
    order = np.argsort(prev["ids"], kind="stable")
    prev = {k: np.ascontiguousarray(v[order]) for k, v in prev.items()}
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R0, T0
    if pose_noise:
        T[:3, 3] += rng.normal(0, pose_noise, 3)
    return dict(fr=frame(ukp, desc, intr), table=table, prev=prev, local_ids=local["ids"].copy(), pose0=np.ascontiguousarray(T.astype(np.float32).reshape(16)),
                intr=np.array([FX, FY, CX, CY], np.float32))


def depths(sc, seed, frac=0.6, intr=None):
    """Per keypoint: the camera z of a table point that projects onto it (0.5 % noise), else a depth drawn in [4, 40); then none (0 or
    < 0) for a fraction 1 - frac of the keypoints.  intr: the camera that projects (default: the scene's own)."""
    FX, FY, CX, CY = _camera(sc["intr"] if intr is None else intr)
    rng = np.random.default_rng(500 + seed)
    kp = sc["fr"]["und_kpts"]
    n = len(kp)
    d = rng.uniform(4, 40, n)
    Xc = sc["table"]["pos3d"].astype(np.float64) @ R0.T + T0
    u = Xc[:, 0] / Xc[:, 2] * FX + CX
    v = Xc[:, 1] / Xc[:, 2] * FY + CY
    if n:
        k = np.rint(u).astype(np.int64) * 1000 + np.rint(v).astype(np.int64)
        lut = dict(zip(k.tolist(), Xc[:, 2].tolist()))
        for i in range(n):
            zz = lut.get(int(np.rint(kp["x"][i])) * 1000 + int(np.rint(kp["y"][i])))
            if zz is not None:
                d[i] = zz * (1 + rng.normal(0, 0.005))
    d[rng.random(n) >= frac] = 0.0
    d[rng.random(n) < 0.02] = -1.0
    return d.astype(np.float32)


def hip_inputs(sc):
    """What uh_track_pose takes, derived from the table by id: the previous-frame items' positions, their rows in the local map
    (prev_map_row), the local map's arrays and weights, the weights of the previous-frame items (uh_track_stereo::prev_weight)."""
    t = sc["table"]
    row_of_id = {int(v): i for i, v in enumerate(t["ids"])}
    local_row = {int(v): i for i, v in enumerate(sc["local_ids"])}
    tr = np.array([row_of_id[int(v)] for v in sc["prev"]["ids"]], np.int64)
    lr = np.array([row_of_id[int(v)] for v in sc["local_ids"]], np.int64)
    w = np.where(t["stable"] != 0, np.float32(1), np.float32(0.5)).astype(np.float32)
    prev = dict(ids=sc["prev"]["ids"], pos3d=np.ascontiguousarray(t["pos3d"][tr].reshape(-1, 3)), octave=sc["prev"]["octave"], desc=sc["prev"]["desc"])
    mp = {k: np.ascontiguousarray(t[k][lr]) for k in ("ids", "pos3d", "normal", "min_dist", "max_dist", "desc")}
    prev_row = np.array([local_row.get(int(v), -1) for v in sc["prev"]["ids"]], np.int32)
    return dict(prev=prev, mp=mp, prev_row=prev_row, map_weight=np.ascontiguousarray(w[lr]), prev_weight=np.ascontiguousarray(w[tr]))


def _prev_with_pos(sc):
    t = sc["table"]
    row_of_id = {int(v): i for i, v in enumerate(t["ids"])}
    tr = np.array([row_of_id[int(v)] for v in sc["prev"]["ids"]], np.int64)
    return dict(ids=sc["prev"]["ids"], pos3d=np.ascontiguousarray(t["pos3d"][tr].reshape(-1, 3)), octave=sc["prev"]["octave"], desc=sc["prev"]["desc"]), tr


def shift_point(sc, table_row, rng, lo=6.0, hi=10.0, intr=None):
    """Move one table point so that it projects lo..hi px from where it did at pose0 (inside the 15 px disc, chi2 above 5.99 at octave 0).
    intr: the camera that projects (default: the scene's own)."""
    FX, FY, _, _ = _camera(sc["intr"] if intr is None else intr)
    P = sc["pose0"].reshape(4, 4).astype(np.float64)
    R, t = P[:3, :3], P[:3, 3]
    Xc = R @ sc["table"]["pos3d"][table_row].astype(np.float64) + t
    ang = rng.uniform(0, 2 * np.pi)
    d = rng.uniform(lo, hi)
    Xc[0] += d * np.cos(ang) / FX * Xc[2]
    Xc[1] += d * np.sin(ang) / FY * Xc[2]
    sc["table"]["pos3d"][table_row] = (R.T @ (Xc - t)).astype(np.float32)


def with_first_search(L, sc, n_match, n_out, octave0_outliers=True, seed=0):
    """Keep only previous-frame items that the first search matches, exactly n_match of them, and shift n_out of those (octave 0 when
    octave0_outliers) so that the first solve relabels them.  Returns the scene (modified in place) and the shifted items' ids."""
    import oracle_lib

    rng = np.random.default_rng(900 + seed)
    pv, _ = _prev_with_pos(sc)
    m = oracle_lib.proj_match_prev(L, sc["fr"], pv, sc["pose0"], 75.0, 15.0)["matches"]
    ids = m["trainIdx"].astype(np.uint32)
    oct_of = {int(v): int(o) for v, o in zip(sc["prev"]["ids"], sc["prev"]["octave"])}
    cand_out = [int(v) for v in ids if (oct_of[int(v)] == 0 or not octave0_outliers)]
    assert len(ids) >= n_match and len(cand_out) >= n_out, (len(ids), len(cand_out), n_match, n_out)
    out = set(rng.choice(cand_out, n_out, replace=False).tolist()) if n_out else set()
    rest = [int(v) for v in ids if int(v) not in out]
    keep = set(out) | set(rng.choice(rest, n_match - n_out, replace=False).tolist())
    sel = np.array([int(v) in keep for v in sc["prev"]["ids"]])
    sc["prev"] = {k: np.ascontiguousarray(v[sel]) for k, v in sc["prev"].items()}
    row_of_id = {int(v): i for i, v in enumerate(sc["table"]["ids"])}
    for v in sorted(out):
        shift_point(sc, row_of_id[v], rng)
    return sc, out
