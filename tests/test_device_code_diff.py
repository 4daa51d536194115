"""tools/device_code_diff.py on a few lines of synthetic assembly: renumbered local labels compare equal, one changed
instruction is reported with its function, a function that exists on one side only is reported."""
import importlib.util
import os

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location("device_code_diff", os.path.join(HERE, "..", "tools", "device_code_diff.py"))
dcd = importlib.util.module_from_spec(spec)
spec.loader.exec_module(dcd)


def kernel(name, n, add="v_add_f64 v[0:1], v[0:1], v[2:3]", sgprs=10):
    """one kernel as the compiler writes it: body, descriptor inside the function's extent, end label; n = its number in
    the file, which the local labels carry"""
    return f"""\t.protected\t{name}
\t.globl\t{name}
\t.p2align\t8
\t.type\t{name},@function
{name}:                               ; @{name}
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0   ; a comment
\ts_cbranch_scc1 .LBB{n}_2
.Ltmp{7 * n}:
\t{add}
.LBB{n}_2:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.p2align\t6, 0x0
\t.amdhsa_kernel {name}
\t\t.amdhsa_next_free_sgpr {sgprs}
\t.end_amdhsa_kernel
\t.section\t.text.{name},"axG",@progbits,{name},comdat
.Lfunc_end{n}:
\t.size\t{name}, .Lfunc_end{n}-{name}
                                        ; -- End function
"""


TAIL = "\t.type\t__hip_cuid_{h},@object\n__hip_cuid_{h}:\n\t.byte 0\n"
REMARK = ("remark: a.hip:{line}:0: Function Name: {name} [-Rpass-analysis=kernel-resource-usage]\n"
          "remark: a.hip:{line}:0:     VGPRs: {v} [-Rpass-analysis=kernel-resource-usage]\n")


def test_renumbered_labels_and_another_cuid_compare_equal():
    old = kernel("first", 0) + kernel("second", 1) + TAIL.format(h="aa")
    new = kernel("second", 0) + kernel("first", 1) + TAIL.format(h="bb")       # the other order: every number moves
    line, diffs = dcd.compare_source("src", old, new, REMARK.format(line=5, name="first", v=8),
                                     REMARK.format(line=9, name="first", v=8))
    assert diffs == []
    assert line.startswith("src: 2 kernels / 2 device functions in parent, 2 / 2 in branch; 2 identical, 0 differing; "
                           "kernel descriptors differing: 0; resource blocks compared: 1, differing: 0")
    assert "8 instruction lines compared" in line


def test_one_changed_instruction_is_reported_with_its_function():
    old = kernel("first", 0) + kernel("second", 1)
    new = kernel("first", 0) + kernel("second", 1, add="v_mul_f64 v[0:1], v[0:1], v[2:3]")
    line, diffs = dcd.compare_source("src", old, new)
    assert "1 identical, 1 differing" in line
    assert len(diffs) == 1 and "second" in diffs[0] and "first" not in diffs[0]
    assert "v_add_f64" in diffs[0] and "v_mul_f64" in diffs[0]
    # ... and a descriptor or a resource block that moved, likewise
    _, diffs = dcd.compare_source("src", old, kernel("first", 0, sgprs=12) + kernel("second", 1),
                                  REMARK.format(line=5, name="second", v=8), REMARK.format(line=5, name="second", v=9))
    assert len(diffs) == 2 and "first kernel descriptor" in diffs[0] and "second resource usage" in diffs[1]


def test_a_function_on_one_side_only_is_reported(tmp_path, capsys):
    old_dir, new_dir = tmp_path / "old", tmp_path / "new"
    old_dir.mkdir()
    new_dir.mkdir()
    (old_dir / ("src" + dcd.ASM_SUFFIX)).write_text(kernel("first", 0) + kernel("gone", 1))
    (new_dir / ("src" + dcd.ASM_SUFFIX)).write_text(kernel("first", 0) + kernel("added", 1))
    (old_dir / ("only_old" + dcd.ASM_SUFFIX)).write_text(kernel("first", 0))
    assert dcd.main(["device_code_diff.py", str(old_dir), str(new_dir)]) == 1
    out = capsys.readouterr().out
    assert "ALL IDENTICAL" not in out
    assert "src: gone exists only in the parent" in out and "src: added exists only in the branch" in out
    assert "only_old: source exists only in the parent" in out
    # the same tree against itself
    assert dcd.main(["device_code_diff.py", str(old_dir), str(old_dir)]) == 0
    assert capsys.readouterr().out.rstrip().endswith("ALL IDENTICAL")
