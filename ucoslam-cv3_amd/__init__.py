"""MI355X-native tracking hot path of UcoSLAM (ORB extract -> Hamming kNN / BoW -> LM/Schur BA).

The product is the HIP library `libucoslam_hip.so` behind the C ABI of include/ucoslam_hip.h;
this package is the thin Python host side used by tests/, bench.py and __graft_entry__.py.
"""
from ._lib import Context, UcoslamHipError, lib  # noqa: F401
from . import ba, bow, fuse, knn, mapinit, matcher, newpoints, orb, parallel, pnp, pnp_ransac, posegraph, projmatch, relocalize, slm, stereo  # noqa: F401,E402  (registers the ctypes prototypes)
from .pnp_ransac import PnPRansac, ransac_samples  # noqa: F401,E402
from .relocalize import relocalize_pose, relocalize_pose_onecall  # noqa: F401,E402
from .fuse import FuseSearch, search_in_neighbors  # noqa: F401,E402
from .mapinit import MapInit, initialize_host, mapinit_samples  # noqa: F401,E402
