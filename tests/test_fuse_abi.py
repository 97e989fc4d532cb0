"""The fuse search at the drop-in boundary: its symbols are exported, the structs its calls take have the header's layout, the status
codes of header, kernel arithmetic and Python mirror agree, and without a GPU the device entry fails loudly while the host form works."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "ucoslam_hip.h")
LIB = os.path.join(ROOT, "ucoslam-cv3_amd", "libucoslam_hip.so")
SYMBOLS = ["uh_fuse_create", "uh_fuse_destroy", "uh_fuse_max_points", "uh_fuse_set_points", "uh_fuse_update_points", "uh_fuse_search", "uh_fuse_search_host"]


def test_symbols_declared_and_exported():
    hdr = open(HDR).read()
    L = C.CDLL(LIB)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert hasattr(L, s), s
    L.uh_fuse_max_points.restype = C.c_int32
    assert L.uh_fuse_max_points() == 1 << 20


def test_struct_sizes():
    from ucoslam_cv3_amd.projmatch import _MapPoints, _ProjFrame

    # uh_map_points: int32 n (+ 4 padding), six pointers; uh_proj_frame: pointer, int32, pointer, pointer, int32, 4 floats, 4 int32
    assert C.sizeof(_MapPoints) == 8 + 6 * 8
    assert C.sizeof(_ProjFrame) == 8 + 8 + 8 + 8 + 4 + 16 + 16 + 4
    assert _MapPoints.pos3d.offset == 16 and _ProjFrame.scale_factors.offset == 24 and _ProjFrame.fx.offset == 36


def test_status_codes_agree():
    from ucoslam_cv3_amd import fuse as UF

    hdr = open(HDR).read()
    codes = {k: int(v) for k, v in re.findall(r"#define UH_FUSE_([A-Z_]+)\s+(\d+)", hdr)}
    assert codes == dict(FOUND=0, SKIPPED=1, NO_PROJECT=2, DISTANCE=3, VIEW_COS=4, NO_KEYPOINT=5)
    assert (UF.FOUND, UF.SKIPPED, UF.NO_PROJECT, UF.DISTANCE, UF.VIEW_COS, UF.NO_KEYPOINT) == (0, 1, 2, 3, 4, 5)
    math = open(os.path.join(ROOT, "ucoslam-cv3_amd", "csrc", "fuse_math.hpp")).read()
    for name, val in (("kFound", 0), ("kSkipped", 1), ("kNoProject", 2), ("kDistance", 3), ("kViewCos", 4), ("kNoKeypoint", 5)):
        assert re.search(r"\b%s = %d," % (name, val), math), name


def test_package_exports():
    import ucoslam_cv3_amd as u

    assert callable(u.search_in_neighbors) and u.FuseSearch is u.fuse.FuseSearch
