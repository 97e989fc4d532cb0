"""What tests/test_fuse_host.py and tests/test_fuse.py share: the constructed problems, the oracle's outcome of each (computed once per
session and left unchanged) and the parity bar — best_kp, best_dist and status equal for every point, bit for bit."""
import numpy as np

import fuse_cases as FC
import fuse_oracle as O

PROBLEMS = FC.problems()
_ORACLE = {}


def oracle_result(name):
    """The oracle's outcome of a problem, computed once per session and shared (tests/test_fuse.py uses it too)."""
    if name not in _ORACLE:
        p = PROBLEMS[name]
        _ORACLE[name] = O.search(p["points"], p["frame"], p["pose"], p["predict_sf"], p["points"]["skip"], p["th"], p["widen"], p["max_desc_dist"], with_info=True)
    return _ORACLE[name]


def assert_equal_outputs(got, ref, names, what):
    for k in ("status", "best_kp", "best_dist"):
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        bad = np.nonzero(a.view(np.uint32 if a.dtype == np.float32 else a.dtype) != b.view(np.uint32 if b.dtype == np.float32 else b.dtype))[0]
        assert len(bad) == 0, f"{what}: {k} differs at " + ", ".join(f"{names[i]} (got {a[i]}, oracle {b[i]})" for i in bad[:8])
