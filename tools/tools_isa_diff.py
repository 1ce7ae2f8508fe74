"""Instruction text of two builds side by side, from two gfx950 assembly files
(hipcc --cuda-device-only -S; works without a GPU):

    python tools/tools_isa_diff.py parent.s branch.s

One verdict per function: `same` when both builds hold it with the same lines in
the same order, `DIFF` otherwise; `gone` / `new` for a function only one build
has.  Compared after dropping `;` comments and the function index inside the
.LBB<n>_, .Ltmp and .Lfunc_ labels, which only count a function's place in its
file.  Exit status 1 when a function both builds have differs."""
import re
import sys


def functions(path):
    """name -> normalised lines between the label of a `.type name,@function` and its .Lfunc_end"""
    out, name, typed = {}, None, set()
    for line in open(path, errors="replace"):
        line = line.split(";")[0].rstrip()
        line = re.sub(r"\.LBB\d+_", ".LBB_", line)
        line = re.sub(r"\.(Ltmp|Lfunc_begin|Lfunc_end)\d+", r".\1", line)
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            typed.add(m.group(1))
        if name is None and line.endswith(":") and line[:-1] in typed:
            name = line[:-1]
            out[name] = []
        elif name is not None:
            if line.strip():
                out[name].append(line)
            if line.startswith(".Lfunc_end"):
                name = None
    return out


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    differ = 0
    for name in sorted(set(a) | set(b)):
        verdict = "new" if name not in a else "gone" if name not in b else "same" if a[name] == b[name] else "DIFF"
        differ += verdict == "DIFF"
        lines = len(b[name]) if name in b else len(a[name])
        print(f"{verdict:5s} {lines:7d} lines  {name}")
    print(f"# functions of both builds that differ: {differ}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
