"""CPU oracle of the mapper's fuse step, written from the reference's text (src/utils/mapmanager.cpp: the private member of MapManager
that is ORB-SLAM's SearchInNeighbors; map.cpp:114-130, 165-185, 264-276, 849-930; map.h:203-233; frame.h:129-159, 189-197; frame.cpp:102-115,
160-166; mappoint.h:99, 146-163) in numpy float32 / float64 scalars — NOT from csrc/fuse_math.hpp.  The candidate lists in picoflann's
order come from oracle_kd_build / oracle_kd_radius (oracle/proj_oracle.cpp) as they are; logf is the host libm's through ctypes.

`search` is one projection search (what uh_fuse_search / uh_fuse_search_host compute); `search_in_neighbors` is the whole function on a
dict-based map, point by point with every event applied at once, exactly as the reference runs it.

Map model (shared with ucoslam_cv3_amd.fuse and tests/host_helpers/toy_fuse_map.hpp):
  map["keyframes"][idx]  = dict(idx, pose_f2g [4,4] f32, und_kpts KEYPOINT_DTYPE[n], desc [n,32] u8, ids uint32[n] (NO_ID = none),
                                scale_factors f32[L], fx, fy, cx, cy, min_xy, max_xy, bad)
  map["map_points"][id]  = dict(id, pos3d f32[3], normal f32[3], min_dist f32, max_dist f32, desc u8[32], frames {frame idx: keypoint}, bad)
  map["neighbors"][idx]  = iterable of keyframe indices (TheKpGraph.getNeighbors)
"""
import copy
import ctypes as C
import ctypes.util

import numpy as np

import oracle_lib

F = np.float32
NO_ID = 0xFFFFFFFF
FOUND, SKIPPED, NO_PROJECT, DISTANCE, VIEW_COS, NO_KEYPOINT = range(6)

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype = C.c_float
_libm.logf.argtypes = [C.c_float]


def logf(x):
    return F(_libm.logf(C.c_float(float(x))))


def camera_center(pose_f2g):
    """Frame::getCameraCenter (frame.h:189-197)."""
    p = np.ascontiguousarray(pose_f2g, F).reshape(16)
    return np.array([-(p[3] * p[0] + p[7] * p[4] + p[11] * p[8]),
                     -(p[3] * p[1] + p[7] * p[5] + p[11] * p[9]),
                     -(p[3] * p[2] + p[7] * p[6] + p[11] * p[10])], F)


def norm3(v):
    """cv::norm(Point3f): double."""
    x, y, z = (np.float64(c) for c in v)
    return np.sqrt(x * x + y * y + z * z)


def project(fr, pose_f2g, p):
    """Frame::project(p, true, true): (x, y) float32 or None for NaN."""
    rt = np.ascontiguousarray(pose_f2g, F).reshape(16)
    with np.errstate(all="ignore"):
        z = p[0] * rt[8] + p[1] * rt[9] + p[2] * rt[10] + rt[11]
        if z < 0:
            return None
        x = p[0] * rt[0] + p[1] * rt[1] + p[2] * rt[2] + rt[3]
        y = p[0] * rt[4] + p[1] * rt[5] + p[2] * rt[6] + rt[7]
        z = F(np.float64(1.) / np.float64(z))
        px = ((F(fr["fx"]) * x) * z) + F(fr["cx"])
        py = ((F(fr["fy"]) * y) * z) + F(fr["cy"])
        if not (px >= F(fr["min_xy"][0]) and py >= F(fr["min_xy"][1]) and px < F(fr["max_xy"][0]) and py < F(fr["max_xy"][1])):
            return None
    return px, py


def view_cos(cc, pos, normal):
    """MapPoint::getViewCos (mappoint.h:99)."""
    v = cc - pos
    s = np.float64(1.) / norm3(v)
    v = np.array([F(np.float64(c) * s) for c in v], F)
    return v[0] * normal[0] + v[1] * normal[1] + v[2] * normal[2]


def predict_scale(scale_factors, dist, maxd):
    """Frame::predictScale (frame.h:129-136)."""
    log_sf = logf(scale_factors[1])
    ns = int(np.ceil(logf(maxd / dist) / log_sf))
    if ns < 0:
        return 0
    if ns >= len(scale_factors):
        return len(scale_factors) - 1
    return ns


def hamming(a, b):
    return F(int(np.unpackbits(np.bitwise_xor(a, b)).sum()))


def desc_threshold(max_desc_dist):
    """pair<float,int> best(maxDescDistance + 1e-3, -1): float + double, stored as float."""
    return F(np.float64(F(max_desc_dist)) + 1e-3)


class FrameKd:
    """The frame's kd-tree (Frame::create_kdtree) behind getKeyPointsInRegion."""

    def __init__(self, fr):
        k = fr["und_kpts"]
        xy = np.stack([k["x"], k["y"]], 1).astype(F) if len(k) else np.zeros((0, 2), F)
        self.kd = oracle_lib.KdOracle(oracle_lib.load_oracle(), "oracle_kd", xy)
        self.octave = np.asarray(k["octave"])

    def region(self, px, py, radius, lo, hi):
        idx, _ = self.kd.radius(px, py, float(radius))
        return [int(i) for i in idx if lo <= self.octave[i] <= hi]


def search_point(fr, kd, pose_f2g, cc, predict_sf, pos, normal, mind, maxd, desc, th, widen, thr, info=None):
    """The loop body for one point against one frame: (status, best keypoint, best distance)."""
    p2d = project(fr, pose_f2g, pos)
    if p2d is None:
        return NO_PROJECT, -1, thr
    dist = F(norm3(cc - pos))
    if dist < F(0.8) * mind or dist > F(1.2) * maxd:
        return DISTANCE, -1, thr
    vc = view_cos(cc, pos, normal)
    if vc < 0.5:
        return VIEW_COS, -1, thr
    level = predict_scale(predict_sf, dist, maxd)
    radius = F(th) * fr["scale_factors"][level]
    if vc < 0.98:
        radius = radius * F(widen)
    cand = kd.region(p2d[0], p2d[1], radius, level - 1, level)
    best_d, best = thr, -1
    dists = []
    for kp in cand:
        d = hamming(desc, fr["desc"][kp])
        dists.append(float(d))
        if d < best_d:
            best_d, best = d, kp
    if info is not None:
        info.update(level=level, radius=float(radius), view_cos=float(vc), dist=float(dist), n_cand=len(cand), cand=cand, cand_dist=dists, p2d=(float(p2d[0]), float(p2d[1])))
    return (FOUND if best != -1 else NO_KEYPOINT), best, best_d


def search(points, fr, pose_f2g, predict_sf, skip=None, th=2.5, widen=1.4, max_desc_dist=100.0, with_info=False):
    """One search: dict(best_kp int32[n], best_dist f32[n], status u8[n][, info list])."""
    n = len(points["pos3d"])
    kd = FrameKd(fr)
    cc = camera_center(pose_f2g)
    sf = np.ascontiguousarray(predict_sf, F)
    thr = desc_threshold(max_desc_dist)
    th = 2.5 if th == 0 else th
    best_kp, best_d, status, infos = np.full(n, -1, np.int32), np.full(n, thr, F), np.zeros(n, np.uint8), []
    for m in range(n):
        info = {}
        if skip is not None and skip[m]:
            st, kp, d = SKIPPED, -1, thr
        else:
            st, kp, d = search_point(fr, kd, pose_f2g, cc, sf, points["pos3d"][m].astype(F), points["normal"][m].astype(F), F(points["min_dist"][m]),
                                     F(points["max_dist"][m]), points["desc"][m], th, widen, thr, info)
        best_kp[m], best_d[m], status[m] = kp, d, st
        infos.append(info)
    out = dict(best_kp=best_kp, best_dist=best_d, status=status)
    if with_info:
        out["info"] = infos
    return out


# ------------------------------------------------------------------------------------------------ the map's own functions (map.cpp)
def update_point_info(mp_map, pid):
    """Map::updatePointInfo = updatePointNormalAndDistances (map.cpp:849-891) + the representative descriptor (:892-930)."""
    kfs = mp_map["keyframes"]
    mp = mp_map["map_points"][pid]
    p3d = mp["pos3d"]
    avg = np.zeros(3, F)
    norm_sum = np.float64(0)
    best = None   # (octave, frame, kp): the first observation of the strictly lowest octave, frames in ascending index
    for f in sorted(mp["frames"]):
        kp = mp["frames"][f]
        normal = camera_center(kfs[f]["pose_f2g"]) - p3d
        avg = avg + normal
        norm_sum = norm_sum + norm3(normal)
        octv = int(kfs[f]["und_kpts"]["octave"][kp])
        if best is None or best[0] > octv:
            best = (octv, f, kp)
    s = np.float64(1.) / norm_sum
    mp["normal"] = np.array([F(np.float64(c) * s) for c in avg], F)
    bf = kfs[best[1]]
    dist = F(norm3(p3d - camera_center(bf["pose_f2g"])))
    maxd = dist * bf["scale_factors"][best[0]]
    mp["max_dist"] = F(maxd)
    mp["min_dist"] = F(maxd / bf["scale_factors"][-1])
    obs = [(f, mp["frames"][f]) for f in sorted(mp["frames"])]
    k = len(obs)
    dd = np.zeros((k, k), F)
    for i in range(k):
        for j in range(i + 1, k):
            dd[i, j] = dd[j, i] = hamming(kfs[obs[i][0]]["desc"][obs[i][1]], kfs[obs[j][0]]["desc"][obs[j][1]])
    best_r, best_sum = -1, np.finfo(F).max
    for r in range(k):
        sm = F(0)
        for c in range(k):
            sm = sm + dd[r, c]
        if sm < best_sum:
            best_r, best_sum = r, sm
    mp["desc"] = kfs[obs[best_r][0]]["desc"][obs[best_r][1]].copy()


def add_map_point_observation(mp_map, pid, fidx, kp):
    """Map::addMapPointObservation (map.cpp:114-130) without the covisibility graph's edge weights."""
    mp_map["keyframes"][fidx]["ids"][kp] = pid
    mp_map["map_points"][pid]["frames"][fidx] = kp
    update_point_info(mp_map, pid)


def remove_point(mp_map, pid):
    """Map::removePoint(pid, false) (map.cpp:165-185)."""
    mp = mp_map["map_points"][pid]
    mp["bad"] = True
    for f, kp in mp["frames"].items():
        if mp_map["keyframes"][f]["ids"][kp] == pid:
            mp_map["keyframes"][f]["ids"][kp] = NO_ID


def fuse_map_points(mp_map, mp1, mp2):
    """Map::fuseMapPoints(mp1, mp2, false) (map.cpp:264-276): mp2 disappears into mp1."""
    obs2 = dict(mp_map["map_points"][mp2]["frames"])
    remove_point(mp_map, mp2)
    for f in sorted(obs2):
        if f not in mp_map["map_points"][mp1]["frames"]:
            add_map_point_observation(mp_map, mp1, f, obs2[f])


def get_map_points_in_frames(mp_map, frames):
    """Map::getMapPointsInFrames (map.h:203-233): ascending ids of the existing, non-bad points the non-bad frames observe."""
    used = set()
    for f in frames:
        kf = mp_map["keyframes"].get(f)
        if kf is None or kf["bad"]:
            continue
        used.update(int(i) for i in kf["ids"] if i != NO_ID)
    return [i for i in sorted(used) if i in mp_map["map_points"] and not mp_map["map_points"][i]["bad"]]


def search_in_neighbors(mp_map, cur_idx, max_desc_dist, th=2.5):
    """The whole function on mp_map (modified in place).  Returns (removed ids, log); log["events"] lists (half, keyframe, point, 'add' /
    'fuse', keypoint, fusion target or -1) in the order applied, log["state_dependent"] the (keyframe, point) pairs of the first half whose
    outcome differs from what the point's ENTRY state would have given in the same keyframe."""
    kfs, mps = mp_map["keyframes"], mp_map["map_points"]
    cur = kfs[cur_idx]
    entry = copy.deepcopy(mps)
    targets = sorted(f for f in set(mp_map["neighbors"][cur_idx]) if not kfs[f]["bad"])
    removed, events, dependent = [], [], []
    thr = desc_threshold(max_desc_dist)
    pts = [int(i) for i in cur["ids"] if i != NO_ID]
    kds = {}

    def body(half, kf, pid, widen):
        mp = mps[pid]
        if kf["idx"] not in kds:
            kds[kf["idx"]] = FrameKd(kf)
        cc = camera_center(kf["pose_f2g"])
        st, kp, _ = search_point(kf, kds[kf["idx"]], kf["pose_f2g"], cc, cur["scale_factors"], mp["pos3d"], mp["normal"], mp["min_dist"], mp["max_dist"], mp["desc"],
                                 th, widen, thr)
        if half == 1:
            e = entry[pid]
            st0, kp0, _ = search_point(kf, kds[kf["idx"]], kf["pose_f2g"], cc, cur["scale_factors"], e["pos3d"], e["normal"], e["min_dist"], e["max_dist"], e["desc"],
                                       th, widen, thr)
            if (st0, kp0) != (st, kp):
                dependent.append((kf["idx"], pid))
        if st != FOUND:
            return
        tgt = int(kf["ids"][kp])
        if tgt != NO_ID:
            fuse_map_points(mp_map, tgt, pid)
            removed.append(pid)
            mp["bad"] = True
            events.append((half, kf["idx"], pid, "fuse", kp, tgt))
        else:
            add_map_point_observation(mp_map, pid, kf["idx"], kp)
            events.append((half, kf["idx"], pid, "add", kp, -1))

    for t in targets:
        kf = kfs[t]
        for pid in pts:
            if pid not in mps or mps[pid]["bad"] or kf["idx"] in mps[pid]["frames"]:
                continue
            body(1, kf, pid, 1.4)
    for pid in get_map_points_in_frames(mp_map, targets):
        if mps[pid]["bad"] or cur_idx in mps[pid]["frames"]:
            continue
        body(2, cur, pid, 1.0)
    return removed, dict(events=events, state_dependent=dependent, targets=targets)


def map_state(mp_map):
    """What the parity bar compares: ids of every keyframe; frames, bad flag, normal, min / max distance and descriptor of every point."""
    out = {}
    for i, kf in sorted(mp_map["keyframes"].items()):
        out[f"kf{i}.ids"] = np.asarray(kf["ids"], np.uint32).tobytes()
    for i, mp in sorted(mp_map["map_points"].items()):
        out[f"mp{i}.frames"] = tuple(sorted((int(f), int(k)) for f, k in mp["frames"].items()))
        out[f"mp{i}.bad"] = bool(mp["bad"])
        out[f"mp{i}.normal"] = np.asarray(mp["normal"], F).tobytes()
        out[f"mp{i}.minmax"] = np.array([mp["min_dist"], mp["max_dist"]], F).tobytes()
        out[f"mp{i}.desc"] = np.asarray(mp["desc"], np.uint8).tobytes()
    return out
