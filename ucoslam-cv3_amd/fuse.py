"""Host-side mirror of the mapper's search-and-fuse step on top of the C ABI (uh_fuse_*).

Reference: src/utils/mapmanager.cpp, the private member of MapManager that returns vector<uint32_t> and takes Frame& (ORB-SLAM's
SearchInNeighbors): every map point of the new keyframe is searched in each covisible neighbour, then every point of the neighbours in
the new keyframe; a hit on a keypoint that already carries a point fuses the two, a hit on a free keypoint adds an observation.

`FuseSearch` wraps ONE projection search (uh_fuse_search on a device frame, uh_fuse_search_host on the calling core).
`search_in_neighbors` composes the whole function on a dict-based map: K + 1 searches, each one's events applied in point order before
the next (Map::addMapPointObservation / fuseMapPoints / removePoint / updatePointInfo / getMapPointsInFrames of src/map.cpp are
restated below, without the covisibility graph's edge weights).

Map model:
  map["keyframes"][idx]  = dict(idx, pose_f2g [4,4] f32, und_kpts KEYPOINT_DTYPE[n], desc [n,32] u8, ids uint32[n] (NO_ID = none),
                                scale_factors f32[L], fx, fy, cx, cy, min_xy, max_xy, bad)
  map["map_points"][id]  = dict(id, pos3d f32[3], normal f32[3], min_dist f32, max_dist f32, desc u8[32], frames {frame idx: keypoint}, bad)
  map["neighbors"][idx]  = iterable of keyframe indices (TheKpGraph.getNeighbors)
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import I, VP, check, lib, np_ptr
from .orb import KEYPOINT_DTYPE, DeviceFrame
from .projmatch import INT_MAX, _MapPoints, _ProjFrame

NO_ID = 0xFFFFFFFF
FOUND, SKIPPED, NO_PROJECT, DISTANCE, VIEW_COS, NO_KEYPOINT = range(6)
F = np.float32


def _declare(L, sig):
    sig("uh_fuse_create", I, VP, C.POINTER(VP))
    sig("uh_fuse_destroy", None, VP)
    sig("uh_fuse_max_points", C.c_int32)
    sig("uh_fuse_set_points", I, VP, C.POINTER(_MapPoints))
    sig("uh_fuse_update_points", I, VP, C.c_int32, VP, C.POINTER(_MapPoints))
    sig("uh_fuse_search", I, VP, VP, C.POINTER(_ProjFrame), VP, VP, C.c_int32, VP, C.c_float, C.c_float, C.c_float, VP, VP, VP)
    sig("uh_fuse_search_host", I, C.POINTER(_MapPoints), C.POINTER(_ProjFrame), VP, VP, C.c_int32, VP, C.c_float, C.c_float, C.c_float, VP, VP, VP)


_lib._EXTRA_DECLS.append(_declare)


def _points_struct(pos3d, normal, min_dist, max_dist, desc):
    n = len(pos3d)
    a = [np.ascontiguousarray(pos3d, F).reshape(n, 3), np.ascontiguousarray(normal, F).reshape(n, 3), np.ascontiguousarray(min_dist, F).reshape(n),
         np.ascontiguousarray(max_dist, F).reshape(n), np.ascontiguousarray(desc, np.uint8).reshape(n, 32)]
    return _MapPoints(n, None, *[np_ptr(x) if n else None for x in a]), a


def _frame_struct(fr, with_arrays):
    s = np.ascontiguousarray(fr["scale_factors"], F)
    keep = [s]
    k = d = None
    if with_arrays:
        k = np.ascontiguousarray(fr["und_kpts"], KEYPOINT_DTYPE)
        d = np.ascontiguousarray(fr["desc"], np.uint8).reshape(len(k), 32) if len(k) else np.zeros((0, 32), np.uint8)
        keep += [k, d]
    n = len(k) if k is not None else 0
    mn, mx = fr.get("min_xy", (0, 0)), fr.get("max_xy", (INT_MAX, INT_MAX))
    f = _ProjFrame(np_ptr(k) if n else None, n, np_ptr(d) if n else None, np_ptr(s), len(s), fr["fx"], fr["fy"], fr["cx"], fr["cy"], int(mn[0]), int(mn[1]), int(mx[0]), int(mx[1]))
    return f, keep


def _outputs(n):
    return np.full(max(n, 1), -1, np.int32), np.zeros(max(n, 1), F), np.zeros(max(n, 1), np.uint8)


def search_host(points, frame, pose_f2g, predict_scale_factors, skip=None, th=2.5, widen=1.4, max_desc_dist=100.0):
    """uh_fuse_search_host: one search on the calling core (no GPU).  points: dict(pos3d, normal, min_dist, max_dist, desc); frame: dict(und_kpts,
    desc, scale_factors, fx, fy, cx, cy[, min_xy, max_xy]).  Returns dict(best_kp int32[n], best_dist f32[n], status u8[n])."""
    mp, keep = _points_struct(points["pos3d"], points["normal"], points["min_dist"], points["max_dist"], points["desc"])
    f, keep2 = _frame_struct(frame, True)
    pose = np.ascontiguousarray(pose_f2g, F).reshape(16)
    sf = np.ascontiguousarray(predict_scale_factors, F)
    n = mp.n
    sk = np.ascontiguousarray(skip, np.uint8) if skip is not None else None
    bk, bd, st = _outputs(n)
    check(lib().uh_fuse_search_host(C.byref(mp), C.byref(f), np_ptr(pose), np_ptr(sf), len(sf), np_ptr(sk) if sk is not None and n else None, float(th), float(widen),
                                    float(max_desc_dist), np_ptr(bk), np_ptr(bd), np_ptr(st)))
    del keep, keep2
    return dict(best_kp=bk[:n], best_dist=bd[:n], status=st[:n])


class FuseSearch:
    """uh_fuse: a point table in pinned memory and one search per call against a device-resident keyframe."""

    def __init__(self, ctx: _lib.Context):
        self.ctx = ctx
        self._h = VP()
        check(lib().uh_fuse_create(ctx.handle, C.byref(self._h)))
        self.n = 0

    def setPoints(self, pos3d, normal, min_dist, max_dist, desc):
        mp, keep = _points_struct(pos3d, normal, min_dist, max_dist, desc)
        check(lib().uh_fuse_set_points(self._h, C.byref(mp)))
        self.n = mp.n
        del keep

    def updatePoints(self, rows, pos3d, normal, min_dist, max_dist, desc):
        """Rewrite the records of `rows` (the k-th new value belongs to rows[k])."""
        r = np.ascontiguousarray(rows, np.int32)
        mp, keep = _points_struct(pos3d, normal, min_dist, max_dist, desc)
        check(lib().uh_fuse_update_points(self._h, len(r), np_ptr(r) if len(r) else None, C.byref(mp)))
        del keep

    def search(self, frame, pose_f2g, predict_scale_factors, dev_frame: DeviceFrame | None = None, skip=None, th=2.5, widen=1.4, max_desc_dist=100.0):
        """uh_fuse_search.  dev_frame: the keyframe resident on the device (its und_kpts are read from `frame` only when its tree is built by
        the host core); None: the arrays of `frame` are uploaded into a frame object of the handle first."""
        f, keep = _frame_struct(frame, dev_frame is None or "und_kpts" in frame)
        pose = np.ascontiguousarray(pose_f2g, F).reshape(16)
        sf = np.ascontiguousarray(predict_scale_factors, F)
        n = self.n
        sk = np.ascontiguousarray(skip, np.uint8) if skip is not None else None
        if sk is not None and len(sk) != n:
            raise ValueError(f"skip: expected {n} bytes, got {len(sk)}")
        bk, bd, st = _outputs(n)
        check(lib().uh_fuse_search(self._h, dev_frame._h if dev_frame is not None else None, C.byref(f), np_ptr(pose), np_ptr(sf), len(sf),
                                   np_ptr(sk) if sk is not None and n else None, float(th), float(widen), float(max_desc_dist), np_ptr(bk), np_ptr(bd), np_ptr(st)))
        del keep
        return dict(best_kp=bk[:n], best_dist=bd[:n], status=st[:n])

    def close(self):
        if self._h:
            lib().uh_fuse_destroy(self._h)
            self._h = VP()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------------ the map's own functions (src/map.cpp)
def camera_center(pose_f2g):
    """Frame::getCameraCenter (frame.h:189-197)."""
    p = np.ascontiguousarray(pose_f2g, F).reshape(16)
    return np.array([-(p[3] * p[0] + p[7] * p[4] + p[11] * p[8]), -(p[3] * p[1] + p[7] * p[5] + p[11] * p[9]), -(p[3] * p[2] + p[7] * p[6] + p[11] * p[10])], F)


def _norm(v):
    v = v.astype(np.float64)
    return np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])   # cv::norm(Point3f)


def _hamming(a, b):
    return F(int(np.unpackbits(a ^ b).sum()))


def updatePointInfo(m, pid):
    """Map::updatePointInfo (map.cpp:892-930) with updatePointNormalAndDistances (:849-891): mean viewing direction (float sum, double norm
    sum), invariance distances from the first observation of the lowest octave, the descriptor with the smallest distance sum."""
    kfs, mp = m["keyframes"], m["map_points"][pid]
    obs = sorted(mp["frames"].items())
    acc, nsum, best = np.zeros(3, F), np.float64(0), None
    for f, kp in obs:
        nv = camera_center(kfs[f]["pose_f2g"]) - mp["pos3d"]
        acc = acc + nv
        nsum = nsum + _norm(nv)
        o = int(kfs[f]["und_kpts"]["octave"][kp])
        if best is None or o < best[0]:
            best = (o, f)
    mp["normal"] = (acc.astype(np.float64) * (np.float64(1) / nsum)).astype(F)
    bf = kfs[best[1]]
    dist = F(_norm(mp["pos3d"] - camera_center(bf["pose_f2g"])))
    mp["max_dist"] = F(dist * bf["scale_factors"][best[0]])
    mp["min_dist"] = F(mp["max_dist"] / bf["scale_factors"][-1])
    k = len(obs)
    dd = np.zeros((k, k), F)
    for i in range(k):
        for j in range(i + 1, k):
            dd[i, j] = dd[j, i] = _hamming(kfs[obs[i][0]]["desc"][obs[i][1]], kfs[obs[j][0]]["desc"][obs[j][1]])
    sums = [F(0)] * k
    for r in range(k):
        for c in range(k):
            sums[r] = F(sums[r] + dd[r, c])
    r = int(np.argmin(np.array(sums, F)))   # (first strict minimum)
    mp["desc"] = kfs[obs[r][0]]["desc"][obs[r][1]].copy()


def addMapPointObservation(m, pid, fidx, kp):
    m["keyframes"][fidx]["ids"][kp] = pid
    m["map_points"][pid]["frames"][fidx] = kp
    updatePointInfo(m, pid)


def removePoint(m, pid):
    """Map::removePoint(pid, false): the point turns bad and leaves the keyframes' id lists; its own frame list stays."""
    mp = m["map_points"][pid]
    mp["bad"] = True
    for f, kp in mp["frames"].items():
        if m["keyframes"][f]["ids"][kp] == pid:
            m["keyframes"][f]["ids"][kp] = NO_ID


def fuseMapPoints(m, mp1, mp2):
    """Map::fuseMapPoints(mp1, mp2, false).  Returns the point whose record changed (mp1)."""
    obs2 = sorted(m["map_points"][mp2]["frames"].items())
    removePoint(m, mp2)
    for f, kp in obs2:
        if f not in m["map_points"][mp1]["frames"]:
            addMapPointObservation(m, mp1, f, kp)


def getMapPointsInFrames(m, frames):
    used = set()
    for f in frames:
        kf = m["keyframes"].get(f)
        if kf is None or kf["bad"]:
            continue
        used.update(int(i) for i in kf["ids"] if i != NO_ID)
    return [i for i in sorted(used) if i in m["map_points"] and not m["map_points"][i]["bad"]]


def _table(m, ids):
    mps = m["map_points"]
    n = len(ids)
    z3, z1, zd = np.zeros(3, F), F(0), np.zeros(32, np.uint8)
    get = lambda i, k, z: mps[i][k] if i in mps else z   # noqa: E731  (an id that names no point is skipped by the mask; its row is never read)
    return (np.array([get(i, "pos3d", z3) for i in ids], F).reshape(n, 3), np.array([get(i, "normal", z3) for i in ids], F).reshape(n, 3),
            np.array([get(i, "min_dist", z1) for i in ids], F).reshape(n), np.array([get(i, "max_dist", z1) for i in ids], F).reshape(n),
            np.array([get(i, "desc", zd) for i in ids], np.uint8).reshape(n, 32))


def search_in_neighbors(m, cur_idx, max_desc_dist, th=2.5, fuser: FuseSearch | None = None, dev_frames=None):
    """The whole function on map `m` (modified in place); returns the removed point ids in the reference's order.
    fuser: a FuseSearch — the searches run on the device, against dev_frames[idx] (DeviceFrame per keyframe index) where given, else through
    the handle's upload path; None: every search runs through uh_fuse_search_host."""
    kfs, mps = m["keyframes"], m["map_points"]
    cur = kfs[cur_idx]
    targets = sorted(f for f in set(m["neighbors"][cur_idx]) if not kfs[f]["bad"])
    removed = []

    def one_search(kf, ids, skip, widen, table, dirty):
        if fuser is None:
            pts = dict(zip(("pos3d", "normal", "min_dist", "max_dist", "desc"), _table(m, ids)))
            return search_host(pts, kf, kf["pose_f2g"], cur["scale_factors"], skip, th, widen, max_desc_dist)
        if table["fresh"]:
            fuser.setPoints(*_table(m, ids))
            table["fresh"] = False
        elif dirty:
            rows = [r for r, i in enumerate(ids) if i in dirty]
            if rows:
                fuser.updatePoints(rows, *_table(m, [ids[r] for r in rows]))
        dirty.clear()
        return fuser.search(kf, kf["pose_f2g"], cur["scale_factors"], (dev_frames or {}).get(kf["idx"]), skip, th, widen, max_desc_dist)

    def apply(kf, ids, res, dirty):
        for row, pid in enumerate(ids):
            if res["status"][row] != FOUND:
                continue
            kp = int(res["best_kp"][row])
            tgt = int(kf["ids"][kp])
            if tgt != NO_ID:
                fuseMapPoints(m, tgt, pid)
                removed.append(pid)
                mps[pid]["bad"] = True
                dirty.add(tgt)
            else:
                addMapPointObservation(m, pid, kf["idx"], kp)
                dirty.add(pid)

    pts = [int(i) for i in cur["ids"] if i != NO_ID]
    table, dirty = dict(fresh=True), set()
    for t in targets:
        kf = kfs[t]
        skip = np.array([1 if (i not in mps or mps[i]["bad"] or kf["idx"] in mps[i]["frames"]) else 0 for i in pts], np.uint8)
        apply(kf, pts, one_search(kf, pts, skip, 1.4, table, dirty), dirty)
    cands = getMapPointsInFrames(m, targets)
    skip = np.array([1 if (mps[i]["bad"] or cur_idx in mps[i]["frames"]) else 0 for i in cands], np.uint8)
    apply(cur, cands, one_search(cur, cands, skip, 1.0, dict(fresh=True), set()), set())
    return removed
