"""Compare the device assembly of two builds kernel by kernel: isa_diff.py A.s [A.s ...] -- B.s [B.s ...]

Each file is gfx950 device assembly as hipcc writes it with --save-temps or -S --offload-device-only.  A file is
cut at its `; -- Begin function NAME` / `; -- End function` markers (the kernel descriptor, .amdhsa_* with the
register and LDS budget, lies inside them); `;` comments and blank lines are dropped, the numbering of local labels
(.LBB<n>_, .Ltmp<n>, .Lfunc_begin<n>, .Lfunc_end<n>) and the per-file __hip_cuid_* symbol are normalised.  The
kernels of each side are the union over its files.  One line per kernel, `same` or `DIFF`, with the instruction-line
counts; a `DIFF` line also says how many normalised lines differ (-only in A, +only in B) and whether an .amdhsa_
line is among them (`descriptor`: the register or LDS budget changed) or not (`code`), and the differing lines
follow it.  Exit status 1 on any difference, on a kernel one side lacks, or on a kernel one side defines twice.
A plain diff: it looks for no particular instruction.

Used to show what moving kernels between translation units did to their code, e.g. the one bf16 ConvNet file
against its units convnet_fwd.hip, convnet_bwd12.hip, convnet_bwd3.hip and convnet_reduce.hip
(profiles/r08/convnet_split, profiles/r09/convnet_units)."""
import difflib
import re
import sys

BEGIN = re.compile(r"; -- Begin function (\S+)")  # a trailing comment of the symbol's first directive
END = re.compile(r"; -- End function")
LABELS = [(re.compile(r"\.LBB\d+_"), ".LBB_"), (re.compile(r"\.Ltmp\d+"), ".Ltmp"),
          (re.compile(r"\.Lfunc_(begin|end)\d+"), r".Lfunc_\1"), (re.compile(r"__hip_cuid_\w+"), "__hip_cuid_")]


def normalise(line):
    line = line.split(";", 1)[0].strip()
    for pat, rep in LABELS:
        line = pat.sub(rep, line)
    return " ".join(line.split())


def kernels(paths):
    """{name: normalised lines} over all files; the names defined more than once."""
    out, twice = {}, []
    for path in paths:
        name, body = None, []
        for raw in open(path):
            m = BEGIN.search(raw)
            if m:
                name, body = m.group(1), []
            elif END.search(raw) and name is not None:
                if name in out:
                    twice.append(name)
                out[name] = body
                name = None
            elif name is not None:
                line = normalise(raw)
                if line:
                    body.append(line)
    return out, twice


def main(argv):
    if "--" not in argv or argv[0] == "--" or argv[-1] == "--":
        print(__doc__)
        return 2
    cut = argv.index("--")
    (a, a2), (b, b2) = kernels(argv[:cut]), kernels(argv[cut + 1:])
    bad = 0
    for side, names in (("A", a2), ("B", b2)):
        for n in names:
            print(f"TWICE on side {side}: {n}")
            bad += 1
    for n in sorted(set(a) | set(b)):
        if n not in a or n not in b:
            print(f"ONLY {'A' if n in a else 'B'}  {n}")
            bad += 1
            continue
        if a[n] == b[n]:
            print(f"same  {len(a[n]):6d} {len(b[n]):6d}  {n}")
            continue
        bad += 1
        delta = []  # the lines only one side has, in order
        for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, a[n], b[n], autojunk=False).get_opcodes():
            if tag != "equal":
                delta += [("-", l) for l in a[n][i1:i2]] + [("+", l) for l in b[n][j1:j2]]
        minus = sum(sign == "-" for sign, _ in delta)
        kind = "descriptor" if any(l.startswith(".amdhsa_") for _, l in delta) else "code"
        print(f"DIFF  {len(a[n]):6d} {len(b[n]):6d}  -{minus} +{len(delta) - minus} {kind}  {n}")
        for sign, l in delta:
            print(f"      {sign} {l}")
    if not a and not b:
        print("no function markers found")
        bad += 1
    print(f"{len(set(a) | set(b))} kernels, {bad} problem(s)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
