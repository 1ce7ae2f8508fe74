"""Kernel resource table of two builds side by side, from two files of hipcc
-Rpass-analysis=kernel-resource-usage remarks (works without a GPU):

    python tools/tools_resource_diff.py parent.rpass branch.rpass [name regex]

One row per kernel: VGPRs, SGPRs, scratch bytes/lane, LDS bytes/block, occupancy,
VGPR and SGPR spills of both builds; `same` / `DIFF` in the last column, `new`
for kernels only the second build has.  Kernels are matched by name and
template arguments."""
import re
import sys

KEYS = (("vgpr", r"\bVGPRs: (\d+)"), ("sgpr", r"TotalSGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
        ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"),
        ("vspill", r"VGPRs Spill: (\d+)"), ("sspill", r"SGPRs Spill: (\d+)"))


def short(name):
    name = re.sub(r"_ZN12_GLOBAL__N_1\d+", "", name)
    name = re.sub(r"^_Z\d+", "", name)
    m = re.match(r"(\w+?)I((?:L[bi]\d+E)+)E", name)
    if m:
        args = re.findall(r"L[bi](\d+)E", m.group(2))
        return f"{m.group(1)}<{','.join(args)}>"
    return re.sub(r"(P|v|\d+HIP).*", "", name) if "<" not in name else name


def parse(path):
    rows, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = rows.setdefault(short(m.group(1)), {})
            continue
        if cur is None:
            continue
        for key, pat in KEYS:
            m = re.search(pat, line)
            if m:
                cur[key] = int(m.group(1))
    return rows


def main():
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    pat = sys.argv[3] if len(sys.argv) > 3 else "."
    cols = [k for k, _ in KEYS]
    print(f"{'kernel':52s} " + " ".join(f"{c:>13s}" for c in cols) + "  verdict")
    differ = 0
    for name in sorted(set(a) | set(b)):
        if not re.search(pat, name):
            continue
        ra, rb = a.get(name), b.get(name)
        cells = []
        for c in cols:
            x = "-" if ra is None else str(ra.get(c, "-"))
            y = "-" if rb is None else str(rb.get(c, "-"))
            cells.append(f"{x + ' | ' + y:>13s}")
        verdict = "new" if ra is None else "gone" if rb is None else "same" if ra == rb else "DIFF"
        differ += verdict in ("DIFF", "gone")
        print(f"{name:52s} " + " ".join(cells) + f"  {verdict}")
    print(f"# cells: first build | second build; kernels that differ or left: {differ}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
