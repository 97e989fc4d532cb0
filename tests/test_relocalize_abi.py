"""uh_relocalize_pose at the drop-in boundary: the symbol is declared and exported, the ctypes mirrors of its structs have the
header's layout (sizeof / offsetof from a small C program compiled against include/ucoslam_hip.h), the stage codes of header and Python
mirror agree, and the package exports the one-call form beside the composed one."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "ucoslam_hip.h")
LIB = os.path.join(ROOT, "ucoslam-cv3_amd", "libucoslam_hip.so")
STRUCTS = {
    "uh_reloc_args": ["intr4", "inv_sigma_levels", "n_levels", "map_min_desc_dist", "map_radius", "max_iters", "min_matches_ransac", "min_matches_after_ransac",
                      "min_matches_map", "min_good"],
    "uh_reloc_candidate": ["n", "query_idx", "p3d", "normal", "rt6_in", "samples", "points", "weight"],
    "uh_reloc_step": ["stage", "ok", "n_inliers", "best_iter", "rt6", "pose_ransac", "inliers", "cap_inliers", "n_map", "matches_map", "bad", "cap_map", "pose_solve",
                      "iters", "solve_inliers", "n_good"],
    "uh_reloc_result": ["best", "pose", "n_matches", "steps"],
}


def test_symbol_declared_and_exported():
    assert re.search(r"\buh_relocalize_pose\s*\(", open(HDR).read())
    assert hasattr(C.CDLL(LIB), "uh_relocalize_pose")


def test_struct_layouts_match_the_header(tmp_path):
    from ucoslam_cv3_amd import relocalize as R

    mirrors = {"uh_reloc_args": R._RelocArgs, "uh_reloc_candidate": R._RelocCandidate, "uh_reloc_step": R._RelocStep, "uh_reloc_result": R._RelocResult}
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "ucoslam_hip.h"', "int main(void) {"]
    for s, fields in STRUCTS.items():
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        lines += ['    printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (s, f, s, f) for f in fields]
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    want = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for s, fields in STRUCTS.items():
        m = mirrors[s]
        assert [f for f, _ in m._fields_] == fields, s
        assert C.sizeof(m) == int(want[s]), (s, C.sizeof(m), want[s])
        for f in fields:
            assert getattr(m, f).offset == int(want["%s.%s" % (s, f)]), (s, f)


def test_stage_codes_agree():
    from ucoslam_cv3_amd import relocalize as R

    m = re.search(r"enum \{ UH_RELOC_FEW_MATCHES = 0, UH_RELOC_FEW_AFTER_RANSAC = 1, UH_RELOC_FEW_MAP = 2, UH_RELOC_FEW_GOOD = 3, UH_RELOC_SOLVED = 4 \};", open(HDR).read())
    assert m and len(R.STAGES) == 5 and R.STAGES[0] == "matches < 25" and R.STAGES[4] == "solved"


def test_package_exports():
    import ucoslam_cv3_amd as u

    assert callable(u.relocalize_pose_onecall) and u.relocalize_pose is u.relocalize.relocalize_pose
