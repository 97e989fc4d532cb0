"""Constructed cases of the fuse search, shared by tests/test_fuse_host.py (host form, no GPU) and tests/test_fuse.py (device).

A frame is built around PLANTED keypoints whose pixel, octave and descriptor are chosen so that each point's outcome names the branch it
took; the rest of the frame is a seeded background that keeps clear of the planted sites.  A problem = frame x view x point list; every
point carries the outcome it was built for (`expect`: status and, where it is the point of the case, the keypoint), which the host
test checks against the oracle ALONE before anything of the library is compared.

Planted sites (pixels of a 640 x 480 image, 8 levels, scale 1.2):
  ISO     kp 0            (100, 100) octave 2, alone within 15 px: threshold cases (distance == maxDescDistance, one more)
  TIE     kp 1, 2         (200, 150), (201.5, 150.5) octave 2: equal Hamming distance, the kd-tree order decides
  WIDE    kp 3, 4         (150, 300), (155.2, 300) octave 3: kp 4 lies between the plain and the widened radius of level 3
  LADDER  kp 5 .. 12      within 1 px of (500, 400), octave k at kp 5 + k, Hamming distance 20 - 2k to DESC_LADDER: the best keypoint of a
                          point with that descriptor IS its predicted level (octaves [level - 1, level], the higher one is nearer)
  DENSE   kp 13 .. 212    200 keypoints within 5 px of (450, 300), octaves 3 / 4: one disc of level 4 lists them all (several drains)
"""
import numpy as np

from oracle_lib import KEYPOINT_DTYPE

F = np.float32
W, H = 640, 480
N_LEVELS = 8
_sf = [F(1)]
for _ in range(N_LEVELS - 1):
    _sf.append(F(_sf[-1] * F(1.2)))
SCALE = np.array(_sf, F)
FX, FY, CX, CY = 512.0, 512.0, 320.0, 240.0
MAX_DESC_DIST = 50.0
SITES = [(100, 100), (200, 150), (150, 300), (500, 400), (450, 300)]
ISO, TIE_A, TIE_B, WIDE_A, WIDE_B, LADDER0, DENSE0, N_PLANTED = 0, 1, 2, 3, 4, 5, 13, 213
FOUND, SKIPPED, NO_PROJECT, DISTANCE, VIEW_COS, NO_KEYPOINT = range(6)


def _flip(desc, bits):
    d = np.unpackbits(desc.copy())
    d[list(bits)] ^= 1
    return np.packbits(d)


_rng0 = np.random.default_rng(20240)
DESC_ISO, DESC_TIE, DESC_WIDE, DESC_LADDER, DESC_DENSE = (_rng0.integers(0, 256, 32, dtype=np.uint8) for _ in range(5))


def make_frame(n, seed):
    """n keypoints (>= N_PLANTED, or 0 / 1 for the degenerate frames)."""
    rng = np.random.default_rng(seed)
    k = np.zeros(n, KEYPOINT_DTYPE)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    if n >= N_PLANTED:
        def put(i, x, y, octv, d):
            k["x"][i], k["y"][i], k["octave"][i] = x, y, octv
            desc[i] = d
        put(ISO, 100, 100, 2, DESC_ISO)
        put(TIE_A, 200, 150, 2, _flip(DESC_TIE, range(0, 10)))
        put(TIE_B, 201.5, 150.5, 2, _flip(DESC_TIE, range(10, 20)))
        put(WIDE_A, 150, 300, 3, _flip(DESC_WIDE, range(0, 30)))
        put(WIDE_B, 155.2, 300, 3, _flip(DESC_WIDE, range(40, 45)))
        for o in range(N_LEVELS):
            put(LADDER0 + o, 500 + 0.1 * o, 400 - 0.1 * o, o, _flip(DESC_LADDER, range(8 * o, 8 * o + 20 - 2 * o)))
        for i in range(200):
            r, a = 4.9 * np.sqrt((i + 0.5) / 200), 2.399963 * i
            k["x"][DENSE0 + i], k["y"][DENSE0 + i], k["octave"][DENSE0 + i] = 450 + r * np.cos(a), 300 + r * np.sin(a), 3 + (i & 1)
        desc[DENSE0 + 37] = _flip(DESC_DENSE, range(0, 7))      # two keypoints at distance 7: the first in kd-tree order wins,
        desc[DENSE0 + 158] = _flip(DESC_DENSE, range(100, 107))  # wherever the drains cut the list
        i = N_PLANTED
        while i < n:
            x, y = rng.uniform(20, W - 20), rng.uniform(20, H - 20)
            if any(abs(x - sx) < 15 and abs(y - sy) < 15 for sx, sy in SITES):
                continue
            k["x"][i], k["y"][i], k["octave"][i] = x, y, rng.integers(0, N_LEVELS)
            i += 1
    elif n == 1:
        k["x"][0], k["y"][0], k["octave"][0] = 320, 240, 2
        desc[0] = DESC_ISO
    k["size"], k["angle"], k["response"], k["class_id"] = 31, -1, 0, -1
    return dict(und_kpts=k, desc=desc, scale_factors=SCALE.copy(), fx=FX, fy=FY, cx=CX, cy=CY, min_xy=(0, 0), max_xy=(W, H))


def _rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def view(kind):
    T = np.eye(4)
    if kind == "general":
        T[:3, :3] = _rot(1, 5) @ _rot(0, -3)
        T[:3, 3] = [0.3, -0.2, 0.5]
    return T.astype(F)


def _cc(T):
    p = T.reshape(16)
    return np.array([-(p[3] * p[0] + p[7] * p[4] + p[11] * p[8]), -(p[3] * p[1] + p[7] * p[5] + p[11] * p[9]), -(p[3] * p[2] + p[7] * p[6] + p[11] * p[10])], F)


def _dist(T, p):
    v = (_cc(T) - p).astype(np.float64)
    return F(np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))


def _nudge(target, start, f):
    """A float32 x near `start` with f(x) == target exactly (searched over +-64 ulps)."""
    x = F(start)
    for step in range(0, 65):
        for cand in {_ulps(x, step), _ulps(x, -step)}:
            if f(cand) == target:
                return cand
    raise AssertionError("no exact float32 solution near %r" % start)


def _ulps(x, k):
    return (np.array([x], F).view(np.int32) + np.int32(k)).view(F)[0]


class _Builder:
    def __init__(self, T):
        self.T, self.rows = T, []

    def add(self, name, expect, u, v, z=4.0, level=4, angle=0.0, desc=None, pos=None, **over):
        T = self.T.astype(np.float64)
        with np.errstate(all="ignore"):
            return self._add(T, name, expect, u, v, z, level, angle, desc, pos, over)

    def _add(self, T, name, expect, u, v, z, level, angle, desc, pos, over):
        if pos is None:
            xc = np.array([(u - CX) / FX * z, (v - CY) / FY * z, z])
            pos = (T[:3, :3].T @ (xc - T[:3, 3])).astype(F)
        pos = np.asarray(pos, F)
        dist = _dist(self.T, pos)
        to_cam = (_cc(self.T) - pos).astype(np.float64)
        to_cam /= np.linalg.norm(to_cam)
        perp = np.cross(to_cam, [0.3, 0.9, 0.1])
        perp /= np.linalg.norm(perp)
        a = np.deg2rad(angle)
        normal = (np.cos(a) * to_cam + np.sin(a) * perp).astype(F)
        maxd = F(dist * F(1.2 ** (level - 0.5))) if level >= 1 else F(dist * F(0.95))
        row = dict(name=name, expect=expect, pos3d=pos, normal=normal, min_dist=F(dist * F(0.5)), max_dist=maxd,
                   desc=np.asarray(desc if desc is not None else DESC_ISO, np.uint8), skip=0, dist=dist)
        row.update(over)
        self.rows.append(row)
        return row


def points_for(T, identity):
    """The point list of a full frame under view T.  identity: the cases that need exact pixel arithmetic (T == eye)."""
    b = _Builder(T)
    # threshold: distance == maxDescDistance is accepted (50 < 50.001), one more is refused
    b.add("thr_equal", (FOUND, ISO), 100, 100, level=2, desc=_flip(DESC_ISO, range(0, 50)))
    b.add("thr_above", (NO_KEYPOINT, -1), 100, 100, level=2, desc=_flip(DESC_ISO, range(0, 51)))
    b.add("iso_found", (FOUND, ISO), 100.4, 99.7, level=3, desc=_flip(DESC_ISO, range(3)))
    b.add("iso_wrong_octave", (NO_KEYPOINT, -1), 100, 100, level=5, desc=DESC_ISO)   # octaves [4, 5]: kp 0 has 2
    # two candidates at the same distance: the first in kd-tree order (the oracle says which)
    b.add("tie", (FOUND, None), 200.7, 150.2, level=2, desc=DESC_TIE)
    # viewCos on either side of 0.98 (radius of level 3: 4.32 plain, 6.05 widened; kp 4 is 5.2 px away) and of 0.5
    b.add("cos_above_098", (FOUND, WIDE_A), 150, 300, level=3, angle=10, desc=DESC_WIDE)
    b.add("cos_below_098", (FOUND, WIDE_B), 150, 300, level=3, angle=13, desc=DESC_WIDE)
    b.add("cos_above_05", (FOUND, WIDE_B), 150, 300, level=3, angle=59, desc=DESC_WIDE)
    b.add("cos_below_05", (VIEW_COS, -1), 150, 300, level=3, angle=61, desc=DESC_WIDE)
    # predicted level read off the ladder: level 0 (octaves [-1, 0]), middle levels, the clamped top
    b.add("level0", (FOUND, LADDER0), 500, 400, level=0, desc=DESC_LADDER)
    for lv in (1, 3, 6):
        b.add(f"level{lv}", (FOUND, LADDER0 + lv), 500, 400, level=lv, desc=DESC_LADDER)
    b.add("level_clamped", (FOUND, LADDER0 + 7), 500, 400, level=9, desc=DESC_LADDER)
    # maxd / dist an exact power of the scale factor: log ratio / log(scale) sits ON an integer, the ceil decides (the oracle says how)
    for k in (1, 2, 3, 5):
        r = b.add(f"exact_power{k}", (FOUND, None), 500, 400, level=k, desc=DESC_LADDER)
        r["max_dist"] = _nudge(SCALE[k], r["dist"] * SCALE[k], lambda m, d=r["dist"]: F(m / d))
    # dist exactly 0.8f * min and exactly 1.2f * max: both kept (the reference's comparisons are strict)
    r = b.add("dist_at_min", (FOUND, LADDER0 + 4), 500, 400, level=4, desc=DESC_LADDER)
    r["min_dist"] = _nudge(r["dist"], r["dist"] / F(0.8), lambda m: F(0.8) * m)
    r = b.add("dist_at_max", (FOUND, LADDER0), 500, 400, level=1, desc=DESC_LADDER)   # log ratio = -1 or just below: level 0 either way
    r["max_dist"] = _nudge(r["dist"], r["dist"] / F(1.2), lambda m: F(1.2) * m)
    r = b.add("dist_below_min", (DISTANCE, -1), 500, 400, level=4, desc=DESC_LADDER)
    r["min_dist"] = F(r["dist"] * F(1.3))
    r = b.add("dist_above_max", (DISTANCE, -1), 500, 400, level=4, desc=DESC_LADDER)
    r["max_dist"] = F(r["dist"] * F(0.8))
    # a disc that lists 200 keypoints: several drains, the tie at distance 7 across them
    b.add("dense", (FOUND, None), 450, 300, level=4, desc=DESC_DENSE)
    b.add("dense_widened", (FOUND, None), 450, 300, level=4, angle=15, desc=DESC_DENSE)
    # projection: behind the camera, outside the image
    b.add("behind", (NO_PROJECT, -1), 320, 240, z=-3.0)
    b.add("outside_left", (NO_PROJECT, -1), -5, 240)
    b.add("outside_bottom", (NO_PROJECT, -1), 320, 481)
    # the caller's mask: one point that would be found, one that would not
    b.add("skip_found", (SKIPPED, -1), 100, 100, level=2, desc=DESC_ISO, skip=1)
    b.add("skip_behind", (SKIPPED, -1), 320, 240, z=-3.0, skip=1)
    if identity:
        # fx = 512, cx = 320, z = 4: x = -2.5 projects on 0 exactly (inside: >= min), x = +2.5 on 640 exactly (outside: < max)
        b.add("on_min_x", (NO_KEYPOINT, -1), 0, 0, pos=[-2.5, 0.0, 4.0])
        b.add("on_max_x", (NO_PROJECT, -1), 0, 0, pos=[2.5, 0.0, 4.0])
        b.add("on_min_y", (NO_KEYPOINT, -1), 0, 0, pos=[0.0, -1.875, 4.0])
        b.add("on_max_y", (NO_PROJECT, -1), 0, 0, pos=[0.0, 1.875, 4.0])
        b.add("z_zero", (NO_PROJECT, -1), 0, 0, pos=[0.5, 0.25, 0.0])
        b.add("z_zero_centre", (NO_PROJECT, -1), 0, 0, pos=[0.0, 0.0, 0.0], normal=np.array([0, 0, -1], F), min_dist=F(0), max_dist=F(1))
    return b.rows


def _table(rows):
    n = len(rows)
    return dict(n=n, names=[r["name"] for r in rows], expect=[r["expect"] for r in rows],
                pos3d=np.array([r["pos3d"] for r in rows], F).reshape(n, 3), normal=np.array([r["normal"] for r in rows], F).reshape(n, 3),
                min_dist=np.array([r["min_dist"] for r in rows], F), max_dist=np.array([r["max_dist"] for r in rows], F),
                desc=np.array([r["desc"] for r in rows], np.uint8).reshape(n, 32), skip=np.array([r["skip"] for r in rows], np.uint8))


def problems():
    """{name: dict(frame, pose, points, predict_sf, th, widen, max_desc_dist)}."""
    out = {}
    for name, n, seed, kind in (("kp300_general", 300, 11, "general"), ("kp2000_identity", 2000, 12, "identity"), ("kp2000_general", 2000, 13, "general")):
        T = view(kind)
        out[name] = dict(frame=make_frame(n, seed), pose=T, points=_table(points_for(T, kind == "identity")), predict_sf=SCALE.copy(), th=2.5, widen=1.4,
                         max_desc_dist=MAX_DESC_DIST)
    T = view("general")
    # second half's form: no widening, th = 0 standing for 2.5
    out["kp300_no_widen"] = dict(frame=make_frame(300, 11), pose=T, points=_table(points_for(T, False)), predict_sf=SCALE.copy(), th=0.0, widen=1.0, max_desc_dist=MAX_DESC_DIST, check_expect=False)
    # the predictor of ANOTHER frame: fewer levels and another scale factor than the searched one
    sf2 = np.array([1, 1.3, 1.69, 2.197, 2.8561], F)
    out["kp300_other_predictor"] = dict(frame=make_frame(300, 11), pose=T, points=_table(points_for(T, False)), predict_sf=sf2, th=2.5, widen=1.4, max_desc_dist=MAX_DESC_DIST, check_expect=False)
    centre = _Builder(T)
    centre.add("centre", (NO_KEYPOINT, -1), 320, 240, level=2, desc=DESC_ISO)
    centre.add("behind", (NO_PROJECT, -1), 320, 240, z=-3.0)
    out["kp0"] = dict(frame=make_frame(0, 1), pose=T, points=_table(centre.rows), predict_sf=SCALE.copy(), th=2.5, widen=1.4, max_desc_dist=MAX_DESC_DIST)
    one = _Builder(T)
    one.add("centre", (FOUND, 0), 320.5, 240.5, level=2, desc=_flip(DESC_ISO, range(4)))
    one.add("centre_far", (NO_KEYPOINT, -1), 330, 240, level=2, desc=DESC_ISO)
    out["kp1"] = dict(frame=make_frame(1, 1), pose=T, points=_table(one.rows), predict_sf=SCALE.copy(), th=2.5, widen=1.4, max_desc_dist=MAX_DESC_DIST)
    out["no_points"] = dict(frame=make_frame(300, 11), pose=T, points=_table([]), predict_sf=SCALE.copy(), th=2.5, widen=1.4, max_desc_dist=MAX_DESC_DIST)
    return out
