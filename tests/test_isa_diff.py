"""scripts/kernel_isa_diff.py on two hand-written assembly files: no compiler, no GPU."""
import os
import subprocess
import sys

TOOL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "kernel_isa_diff.py")

KERNEL = """\
\t.globl\t{name}
\t.type\t{name},@function
{name}: ; @{name}
; %bb.0:
\ts_load_dword s0, s[4:5], 0x0 {comment}
\ts_cbranch_scc1 .LBB{lab}_2
.LBB{lab}_2: ; %exit
\t{op} v0, v1, v2
\ts_endpgm
\t.section\t.rodata
\t.amdhsa_kernel {name}
\t\t.amdhsa_group_segment_fixed_size 64
\t\t.amdhsa_private_segment_fixed_size 0
\t\t.amdhsa_kernarg_size 16
\t\t.amdhsa_next_free_vgpr {vgpr}
\t\t.amdhsa_next_free_sgpr 8
\t\t.amdhsa_accum_offset 4
\t.end_amdhsa_kernel
"""


def _run(tmp_path, a, b):
    pa, pb = tmp_path / "a.s", tmp_path / "b.s"
    pa.write_text(a)
    pb.write_text(b)
    r = subprocess.run([sys.executable, TOOL, str(pa), str(pb), "--show", "4"], capture_output=True, text=True)
    return r.returncode, r.stdout


def test_same_despite_comments_and_label_numbers(tmp_path):
    a = KERNEL.format(name="k_one", lab="0", op="v_add_f32", vgpr=3, comment="") + KERNEL.format(name="k_two", lab="1", op="v_mul_f32", vgpr=3, comment="")
    b = KERNEL.format(name="k_one", lab="7", op="v_add_f32", vgpr=3, comment="; 4-byte Folded Reload") + KERNEL.format(name="k_two", lab="9", op="v_mul_f32", vgpr=3, comment="")
    rc, out = _run(tmp_path, a, b)
    assert rc == 0, out
    lines = out.splitlines()
    assert lines[0].startswith("SAME k_one insns=4 hist=equal") and "vgpr=3" in lines[0] and "lds=64" in lines[0] and "kernarg=16" in lines[0]
    assert lines[1].startswith("SAME k_two")
    assert lines[-1] == "2 kernels, 0 differ"


def test_diff_in_one_instruction(tmp_path):
    a = KERNEL.format(name="k_one", lab="0", op="v_add_f32", vgpr=3, comment="")
    b = KERNEL.format(name="k_one", lab="0", op="v_sub_f32", vgpr=3, comment="")
    rc, out = _run(tmp_path, a, b)
    assert rc == 1
    assert out.splitlines()[0].startswith("DIFF k_one insns=4 hist=differs")
    assert "v_add_f32 v0, v1, v2" in out and "v_sub_f32 v0, v1, v2" in out


def test_diff_in_a_resource_figure_only(tmp_path):
    a = KERNEL.format(name="k_one", lab="0", op="v_add_f32", vgpr=3, comment="")
    b = KERNEL.format(name="k_one", lab="0", op="v_add_f32", vgpr=5, comment="")
    rc, out = _run(tmp_path, a, b)
    assert rc == 1
    assert out.splitlines()[0].startswith("DIFF k_one insns=4 hist=equal") and "vgpr=3->5" in out


def test_kernel_on_one_side_only(tmp_path):
    a = KERNEL.format(name="k_one", lab="0", op="v_add_f32", vgpr=3, comment="")
    rc, out = _run(tmp_path, a, a + KERNEL.format(name="k_new", lab="1", op="v_add_f32", vgpr=3, comment=""))
    assert rc == 1
    assert "ONLY-B k_new" in out and "SAME k_one" in out
