#!/usr/bin/env python
"""The fused tracker frame (uh_track_pose on a scene of tests/track_scenes.py, host in / host out through the Python mirror): wall time per
call without markers and, where the library has uh_track_pose_markers, through that entry with 0 and with 2 markers.  --reps R: R times over."""
import sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import synth
import track_scenes as TS
import ucoslam_cv3_amd as u
from ucoslam_cv3_amd.orb import Camera, DeviceFrame, FeatParams, ORBextractor
from ucoslam_cv3_amd.pnp import PnPSolver
from ucoslam_cv3_amd.projmatch import ProjectionMatcher

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
ctx = u.Context(0, private=True)
ext = ORBextractor(ctx)
ext.setCamera(Camera(TS.FX, TS.FY, TS.CX, TS.CY, ()))
fr = DeviceFrame(ctx).setTreeBuilder(False)
kps, desc, und = ext.extractFrameDev(synth.frame(TS.W, TS.H, seed=5), fr, FeatParams(maxFeatures=2000, nOctaveLevels=8, scaleFactor=1.2))
ukp = kps.copy()
ukp["x"], ukp["y"] = und[:, 0], und[:, 1]
pm = ProjectionMatcher(ctx)
pm.setFrameDev(fr, TS.SF, TS.FX, TS.FY, TS.CX, TS.CY, (0, 0), (TS.W, TS.H), und_kpts=ukp)
sc = TS.scene(ukp, np.ascontiguousarray(desc).reshape(-1, 32), 5, stable_outside=True)
h = TS.hip_inputs(sc)
pnp = PnPSolver(ctx)
common = dict(prev_map_row=h["prev_row"], map_weight=h["map_weight"])
forms = [("uh_track_pose", lambda: pm.trackPose(pnp, sc["pose0"], TS.INTR, TS.INV_SF, h["prev"], h["mp"], **common))]
if hasattr(pm, "trackPoseMarkers"):
    import marker_synth

    T = np.eye(4)
    T[:3, :3], T[:3, 3] = TS.R0, TS.T0
    mk = marker_synth.make_markers(np.random.default_rng(5), T, TS.INTR, 2)
    forms.append(("uh_track_pose_markers, no markers", lambda: pm.trackPoseMarkers(pnp, sc["pose0"], TS.INTR, TS.INV_SF, h["prev"], h["mp"], markers=None, **common)))
    forms.append(("uh_track_pose_markers, 2 markers", lambda: pm.trackPoseMarkers(pnp, sc["pose0"], TS.INTR, TS.INV_SF, h["prev"], h["mp"], markers=mk, **common)))
for name, call in forms:
    for _ in range(10):
        r = call()
    walls = []
    for _ in range(reps):
        t = time.perf_counter()
        for _ in range(100):
            r = call()
        walls.append((time.perf_counter() - t) / 100 * 1e6)
    print(f"{name}: wall per frame [us] {' '.join(f'{w:.1f}' for w in walls)}  (prev {len(r['matches_prev'])}, union {len(r['matches_all'])} matches, iters {r['iters1'].tolist()} {r['iters2'].tolist()}, inliers {r['inliers1']} {r['inliers2']})")
