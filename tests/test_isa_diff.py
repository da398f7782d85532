"""CPU checks of tools/isa_diff.py on small synthetic device assembly (no compiler run): a kernel is the same
under renumbered local labels and changed comments, and differs by one instruction, by its descriptor, or by
being absent."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "isa_diff.py")

KERNEL = """\
	.globl	{name}                          ; -- Begin function {name}
	.p2align	8
	.type	{name},@function
{name}:                                 ; @{name}
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	v_lshlrev_b32_e32 v0, 2, v0             ; {note}
	s_cbranch_scc1 .LBB{n}_2
.Ltmp{t}:
; %bb.1:
	{insn}
.LBB{n}_2:
	s_endpgm
	.section	.rodata,"a",@progbits
	.amdhsa_kernel {name}
		.amdhsa_group_segment_fixed_size 1024
		.amdhsa_next_free_vgpr {vgpr}
		.amdhsa_next_free_sgpr 8
	.end_amdhsa_kernel
	.text
.Lfunc_end{n}:
	.size	{name}, .Lfunc_end{n}-{name}
                                        ; -- End function
	.set {name}.num_vgpr, {vgpr}
"""
TAIL = "\t.type\t__hip_cuid_{cuid},@object\n\t.globl\t__hip_cuid_{cuid}\n"


def asm(names, n0=0, cuid="abc123", note="first", insn="v_add_u32_e32 v1, v0, v0", vgpr=2):
    body = "".join(KERNEL.format(name=k, n=n0 + i, t=7 * n0 + i, note=note, insn=insn, vgpr=vgpr)
                   for i, k in enumerate(names))
    return "\t.text\n" + body + TAIL.format(cuid=cuid)


def run(tmp_path, a_files, b_files):
    paths = []
    for side, files in (("a", a_files), ("b", b_files)):
        paths.append([])
        for i, text in enumerate(files):
            p = tmp_path / f"{side}{i}.s"
            p.write_text(text)
            paths[-1].append(str(p))
    return subprocess.run([sys.executable, TOOL, *paths[0], "--", *paths[1]], capture_output=True, text=True)


def test_renumbered_labels_are_the_same(tmp_path):
    # one file with both kernels against one file each, other label numbers, comments and cuid
    r = run(tmp_path, [asm(["k_one", "k_two"])],
            [asm(["k_two"], n0=5, cuid="ffee00", note="second"), asm(["k_one"], n0=3, cuid="001122")])
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l.split() for l in r.stdout.splitlines()]
    assert [l[0] for l in lines if l[-1] in ("k_one", "k_two")] == ["same", "same"]
    assert "DIFF" not in r.stdout


def test_one_changed_instruction(tmp_path):
    r = run(tmp_path, [asm(["k_one", "k_two"])],
            [asm(["k_one"]), asm(["k_two"], n0=1, insn="v_add_u32_e32 v1, v0, v1")])
    assert r.returncode != 0
    status = {l.split()[-1]: l.split()[0] for l in r.stdout.splitlines() if l.split()[-1] in ("k_one", "k_two")}
    assert status == {"k_one": "same", "k_two": "DIFF"}


def test_changed_vgpr_budget(tmp_path):
    r = run(tmp_path, [asm(["k_one"])], [asm(["k_one"], vgpr=3)])
    assert r.returncode != 0 and "DIFF" in r.stdout


def test_missing_kernel(tmp_path):
    r = run(tmp_path, [asm(["k_one", "k_two"])], [asm(["k_one"])])
    assert r.returncode != 0 and "k_two" in r.stdout
    r = run(tmp_path, [asm(["k_one"])], [asm(["k_one", "k_two"])])
    assert r.returncode != 0 and "k_two" in r.stdout


def test_kernel_defined_twice(tmp_path):
    r = run(tmp_path, [asm(["k_one"])], [asm(["k_one"]), asm(["k_one"], n0=1)])
    assert r.returncode != 0


def diff_fields(stdout, name):
    """(lines only in A, lines only in B, class) of kernel `name`'s DIFF line."""
    (line,) = [l.split() for l in stdout.splitlines() if l.split()[0] == "DIFF" and l.split()[-1] == name]
    return line[3], line[4], line[5]


def test_diff_counts_lines_and_says_code(tmp_path):
    # one instruction replaced: one line on each side; one replaced by two: the listing is one line longer
    r = run(tmp_path, [asm(["k_one", "k_two"])],
            [asm(["k_one"], insn="v_add_u32_e32 v1, v0, v1"),
             asm(["k_two"], n0=1, insn="v_add_u32_e32 v1, v0, v1\n\ts_nop 0")])
    assert r.returncode != 0
    assert diff_fields(r.stdout, "k_one") == ("-1", "+1", "code")
    assert diff_fields(r.stdout, "k_two") == ("-1", "+2", "code")
    assert "- v_add_u32_e32 v1, v0, v0" in r.stdout and "+ s_nop 0" in r.stdout  # the differing lines are listed


def test_diff_says_descriptor(tmp_path):
    # a changed register budget is a descriptor difference, with or without a code difference beside it
    r = run(tmp_path, [asm(["k_one", "k_two"])],
            [asm(["k_one"], vgpr=3), asm(["k_two"], n0=1, vgpr=3, insn="v_add_u32_e32 v1, v0, v1")])
    assert r.returncode != 0
    assert diff_fields(r.stdout, "k_one") == ("-1", "+1", "descriptor")
    assert diff_fields(r.stdout, "k_two") == ("-2", "+2", "descriptor")
    assert "same" not in r.stdout
