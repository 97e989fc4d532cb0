"""The toy map of the whole-function tests (tests/test_fuse_adaptor.py, tests/test_fuse.py): one new keyframe (index 10), four good
neighbours (3, 5, 7, 8), one bad neighbour (6) and 280 map points over 200 world points, built so that every event of the fuse step occurs:

  group   world points   what happens
  ADD1    0 .. 59        a point of keyframe 10 finds a free keypoint in every neighbour: add, first half (four times each)
  FUSE1   60 .. 99       it finds the keypoint of its duplicate (observed in 3 and 5): fuse, first half
  ADD2    100 .. 129     a point of the neighbours (5, 7) finds a free keypoint in keyframe 10: add, second half
  FUSE2   130 .. 149     the duplicate's descriptor comes from the BAD keyframe 6, which is never searched; the point of keyframe 10 is too far
                         from the keypoints of 3 and 7 — the duplicate finds it from the other side: fuse, second half
  SAME    150 .. 159     two points of keyframe 10 choose the same free keypoint of keyframe 3: the first adds, the second fuses into it
  STATE   160 .. 169     added in keyframe 3, the point takes that keypoint's descriptor (and a new normal); only with it does it reach the
                         keypoint of keyframe 5 — the oracle reports each such pair as state-dependent
  TARGET  170 .. 179     the fusion target in keyframe 3 is itself a point of keyframe 10 (its changed record is searched in 5, 7, 8)
  NONE    180 .. 199     points of keyframe 10 that no neighbour shows

Every map point's normal, invariance distances and descriptor are what Map::updatePointInfo gives for its observations (fuse_oracle).
Also here: the binary exchange with tests/host_helpers/fuse_adaptor.cpp (dump_map / load_state)."""
import struct

import numpy as np

import fuse_oracle as O
from fuse_cases import CX, CY, FX, FY, H, SCALE, W, _flip, _rot
from oracle_lib import KEYPOINT_DTYPE

F = np.float32
CUR, GOOD, BAD = 10, (3, 5, 7, 8), 6
MAX_DESC_DIST = 50.0
GROUPS = dict(ADD1=range(0, 60), FUSE1=range(60, 100), ADD2=range(100, 130), FUSE2=range(130, 150), SAME=range(150, 160), STATE=range(160, 170),
              TARGET=range(170, 180), NONE=range(180, 200))


def _pose(rx, ry, t):
    T = np.eye(4)
    T[:3, :3] = _rot(0, rx) @ _rot(1, ry)
    T[:3, 3] = t
    return T.astype(F)


POSES = {10: _pose(1, -2, [0.05, 0.02, 0.1]), 3: _pose(0, 3, [0.4, 0.0, 0.0]), 5: _pose(-2, -3, [-0.4, 0.1, 0.05]), 6: _pose(3, 0, [0.0, 0.4, 0.0]),
         7: _pose(2, 2, [0.3, -0.3, 0.2]), 8: _pose(-1, 1, [-0.2, 0.3, -0.2])}


def scene():
    rng = np.random.default_rng(77)
    gx, gy = np.meshgrid(np.linspace(-1.8, 1.8, 20), np.linspace(-1.3, 1.3, 10))
    world = np.stack([gx.ravel() + rng.uniform(-0.02, 0.02, 200), gy.ravel() + rng.uniform(-0.02, 0.02, 200), 6 + 0.5 * np.sin(gx.ravel()) + 0.3 * gy.ravel()], 1)
    world = world[rng.permutation(200)]
    base = rng.integers(0, 256, (200, 32), dtype=np.uint8)
    kps = {i: [] for i in POSES}     # per keyframe: (x, y, octave, descriptor, map point id or NO_ID)
    points = {}

    def project(i, p):
        T = POSES[i].astype(np.float64)
        c = T[:3, :3] @ p + T[:3, 3]
        return FX * c[0] / c[2] + CX, FY * c[1] / c[2] + CY

    def keypoint(i, j, desc, pid=O.NO_ID, shift=(0.0, 0.0), octave=2):
        u, v = project(i, world[j])
        assert 5 < u < W - 5 and 5 < v < H - 5
        kps[i].append((u + shift[0] + rng.uniform(-0.3, 0.3), v + shift[1] + rng.uniform(-0.3, 0.3), octave, desc, pid))
        return len(kps[i]) - 1

    def point(pid, j, obs, offset=0.0):
        points[pid] = dict(id=pid, pos3d=(world[j] + offset * rng.normal(0, 1, 3)).astype(F), frames=dict(obs), bad=False)

    near = lambda j, k=4: _flip(base[j], rng.choice(256, int(rng.integers(0, k + 1)), replace=False))   # noqa: E731
    nid = iter(range(1000))
    dup = iter(range(1000, 2000))
    for j in GROUPS["ADD1"]:
        pid = next(nid)
        point(pid, j, {CUR: keypoint(CUR, j, near(j), pid)})
        for i in GOOD:
            keypoint(i, j, near(j))
    for j in GROUPS["FUSE1"]:
        pid, did = next(nid), next(dup)
        point(pid, j, {CUR: keypoint(CUR, j, near(j), pid)})
        point(did, j, {3: keypoint(3, j, near(j), did), 5: keypoint(5, j, near(j), did)}, 0.01)
        keypoint(7, j, near(j))
    for j in GROUPS["ADD2"]:
        did = next(dup)
        point(did, j, {5: keypoint(5, j, near(j), did), 7: keypoint(7, j, near(j), did)})
        keypoint(CUR, j, near(j))
    for j in GROUPS["FUSE2"]:
        pid, did = next(nid), next(dup)
        bits = rng.permutation(256)
        c = _flip(base[j], bits[:10])
        point(pid, j, {CUR: keypoint(CUR, j, c, pid)})
        point(did, j, {3: keypoint(3, j, _flip(base[j], bits[10:55]), did), BAD: keypoint(BAD, j, base[j].copy(), did), 7: keypoint(7, j, _flip(base[j], bits[55:100]), did)}, 0.01)
    for j in GROUPS["SAME"]:
        p, q = next(nid), next(nid)
        point(p, j, {CUR: keypoint(CUR, j, near(j), p, (-1.0, 0.0))})
        point(q, j, {CUR: keypoint(CUR, j, near(j), q, (1.0, 0.0))}, 0.005)
        keypoint(3, j, near(j))
    for j in GROUPS["STATE"]:
        pid = next(nid)
        bits = rng.permutation(256)
        point(pid, j, {CUR: keypoint(CUR, j, _flip(base[j], bits[:10]), pid)})
        keypoint(3, j, _flip(base[j], bits[:55]))      # 45 bits from the point's descriptor: found
        keypoint(5, j, _flip(base[j], bits[:95]))      # 85 from the entry descriptor, 40 from keyframe 3's
    for j in GROUPS["TARGET"]:
        t, u = next(nid), next(nid)
        point(t, j, {CUR: keypoint(CUR, j, near(j), t, (-1.0, 0.0)), 3: keypoint(3, j, near(j), t)})
        point(u, j, {CUR: keypoint(CUR, j, near(j), u, (1.0, 0.0))}, 0.005)
        for i in (5, 7, 8):
            keypoint(i, j, near(j))
    for j in GROUPS["NONE"]:
        pid = next(nid)
        point(pid, j, {CUR: keypoint(CUR, j, near(j), pid)})
    keyframes = {}
    for i, lst in kps.items():
        order = rng.permutation(len(lst))          # keypoint order is not construction order
        inv = np.argsort(order)
        k = np.zeros(len(lst), KEYPOINT_DTYPE)
        desc = np.zeros((len(lst), 32), np.uint8)
        ids = np.full(len(lst), O.NO_ID, np.uint32)
        for new, old in enumerate(order):
            k["x"][new], k["y"][new], k["octave"][new], desc[new], ids[new] = lst[old]
        k["size"], k["angle"], k["class_id"] = 31, -1, -1
        for mp in points.values():
            if i in mp["frames"]:
                mp["frames"][i] = int(inv[mp["frames"][i]])
        keyframes[i] = dict(idx=i, pose_f2g=POSES[i], und_kpts=k, desc=desc, ids=ids, scale_factors=SCALE.copy(), fx=FX, fy=FY, cx=CX, cy=CY, min_xy=(0, 0),
                            max_xy=(W, H), bad=(i == BAD))
    m = dict(keyframes=keyframes, map_points=points, neighbors={CUR: [8, 3, BAD, 5, 7]})
    for pid in points:
        points[pid]["normal"], points[pid]["min_dist"], points[pid]["max_dist"], points[pid]["desc"] = np.zeros(3, F), F(0), F(0), np.zeros(32, np.uint8)
        O.update_point_info(m, pid)
    return m


# ------------------------------------------------------------------------------------------------ exchange with fuse_adaptor.cpp
def dump_map(m, cur_idx, max_desc_dist, path):
    """int32 cur, float maxDescDistance, int32 n_kf; per keyframe: int32 idx, bad, n, levels; float pose[16], fx fy cx cy; int32 bounds[4];
    float scale[levels], xy[2n]; int32 octave[n]; u8 desc[32n]; uint32 ids[n].  int32 n_nb, uint32 nb[].  int32 n_mp; per point: uint32 id;
    int32 bad; float pos[3], normal[3], min, max; u8 desc[32]; int32 n_obs; uint32 (frame, keypoint)[n_obs]."""
    with open(path, "wb") as f:
        f.write(struct.pack("<ifi", cur_idx, max_desc_dist, len(m["keyframes"])))
        for i, kf in sorted(m["keyframes"].items()):
            k = kf["und_kpts"]
            f.write(struct.pack("<4i", i, int(kf["bad"]), len(k), len(kf["scale_factors"])))
            f.write(np.ascontiguousarray(kf["pose_f2g"], F).tobytes())
            f.write(struct.pack("<4f4i", kf["fx"], kf["fy"], kf["cx"], kf["cy"], *kf["min_xy"], *kf["max_xy"]))
            f.write(np.ascontiguousarray(kf["scale_factors"], F).tobytes())
            f.write(np.stack([k["x"], k["y"]], 1).astype(F).tobytes())
            f.write(np.ascontiguousarray(k["octave"], np.int32).tobytes())
            f.write(np.ascontiguousarray(kf["desc"], np.uint8).tobytes())
            f.write(np.ascontiguousarray(kf["ids"], np.uint32).tobytes())
        nb = list(m["neighbors"][cur_idx])
        f.write(struct.pack("<i", len(nb)) + np.array(nb, np.uint32).tobytes())
        f.write(struct.pack("<i", len(m["map_points"])))
        for i, mp in sorted(m["map_points"].items()):
            f.write(struct.pack("<Ii", i, int(mp["bad"])))
            f.write(np.concatenate([mp["pos3d"], mp["normal"], [mp["min_dist"], mp["max_dist"]]]).astype(F).tobytes())
            f.write(np.ascontiguousarray(mp["desc"], np.uint8).tobytes())
            obs = sorted(mp["frames"].items())
            f.write(struct.pack("<i", len(obs)) + np.array(obs, np.uint32).reshape(-1).tobytes())


def load_state(m, path):
    """What fuse_adaptor.cpp wrote: (removed ids, map state in fuse_oracle.map_state's form).  m gives the shapes (the entry map)."""
    raw = open(path, "rb").read()
    off = 0

    def take(dtype, n=1):
        nonlocal off
        a = np.frombuffer(raw, dtype, n, off).copy()
        off += a.nbytes
        return a

    removed = take(np.uint32, int(take(np.int32)[0])).tolist()
    out = {}
    for i, kf in sorted(m["keyframes"].items()):
        out[f"kf{i}.ids"] = take(np.uint32, len(kf["ids"])).tobytes()
    for i in sorted(m["map_points"]):
        out[f"mp{i}.bad"] = bool(take(np.int32)[0])
        out[f"mp{i}.normal"] = take(F, 3).tobytes()
        out[f"mp{i}.minmax"] = take(F, 2).tobytes()
        out[f"mp{i}.desc"] = take(np.uint8, 32).tobytes()
        n = int(take(np.int32)[0])
        out[f"mp{i}.frames"] = tuple((int(a), int(b)) for a, b in take(np.uint32, 2 * n).reshape(n, 2))
    assert off == len(raw)
    return removed, out
