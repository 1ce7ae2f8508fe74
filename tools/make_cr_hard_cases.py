#!/usr/bin/env python3
"""Builds tools/cr_mine.cpp, mines the hard cases of the cr_* transcendentals and writes
tests/golden/cr_hard_cases.json.

A hard case is a float32 input at which the host's fp64 library result lies within MARGIN fp64 ulps of
an fp32 rounding boundary.  The eight one-argument functions are mined over every finite float32;
cr_pow over its three call-site families and cr_atan2 over generated unit vectors (sampled, see
DESIGN.md §5).  Each entry records the function, the family, the input bits, the host's fp64 result
bits, the correctly rounded fp32 (mpmath, 320 bits, ties to even on the fp32 grid with denormals), and
`double_rounding` where the host's float, (float)y, is not the correctly rounded one.

    python tools/make_cr_hard_cases.py            # a few minutes on 8 cores
"""
import json
import os
import platform
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tools", "cr_mine.cpp")
FIXTURE = os.path.join(ROOT, "tests", "golden", "cr_hard_cases.json")

MARGIN = 16                      # cr_mine.cpp's MARGIN
ONE_ARGUMENT = ["sin", "cos", "tan", "acos", "atan", "exp", "log", "log2"]
POW_FIT_GRID = (1 << 14, 1 << 14)          # sample_x values x thetaI values
ATAN2_SEED, ATAN2_VECTORS = 0x637231, 1 << 30   # two pairs per vector
PRECISION = 320


def compiler():
    return shutil.which("g++")


def build_miner(outdir):
    exe = os.path.join(outdir, "cr_mine")
    subprocess.check_call([compiler(), "-O2", "-fopenmp", "-ffp-contract=off", SOURCE, "-o", exe])
    return exe


def mine(exe, *args):
    """One cr_mine run: [(family, a_bits, b_bits, y_bits)], sorted by input."""
    env = dict(os.environ)
    env["OMP_NUM_THREADS"] = str(min(16, int(env.get("OMP_NUM_THREADS") or 16), os.cpu_count() or 1))
    out = subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True, env=env).stdout
    rows = []
    for line in out.splitlines():
        fam, a, b, y = line.split()
        rows.append((fam, int(a, 16), int(b, 16), int(y, 16)))
    return rows


def _f32(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def _f64(bits):
    return np.array([bits], np.uint64).view(np.float64)[0]


def round_to_f32_bits(v):
    """An mpmath value rounded to the float32 grid, ties to even, denormals included: its bits."""
    import mpmath as mp
    if v == 0:
        return 0
    sign = 0x80000000 if v < 0 else 0
    v = abs(v)
    e = int(mp.frexp(v)[1]) - 1                 # 2^e <= v < 2^(e+1)
    q = max(e, -126) - 23                       # the grid's spacing there is 2^q
    n = mp.ldexp(v, -q)                         # exact
    lo = mp.floor(n)
    frac = n - lo
    r = int(lo)
    if frac > 0.5 or (frac == 0.5 and (r & 1)):
        r += 1
    value = mp.ldexp(mp.mpf(r), q)              # at most 25 bits: exact in a double
    if value >= mp.ldexp(mp.mpf(1), 128):
        return sign | 0x7f800000
    return sign | int(np.array([float(value)], np.float64).astype(np.float32).view(np.uint32)[0])


def correctly_rounded(fn, a_bits, b_bits):
    import mpmath as mp
    mp.mp.prec = PRECISION
    a, b = mp.mpf(float(_f32(a_bits))), mp.mpf(float(_f32(b_bits)))
    f = {"sin": mp.sin, "cos": mp.cos, "tan": mp.tan, "acos": mp.acos, "atan": mp.atan, "exp": mp.exp, "log": mp.log,
         "log2": lambda x: mp.log(x, 2)}
    if fn == "pow":
        v = mp.power(a, b)
    elif fn == "atan2":
        v = mp.atan2(a, b)
    else:
        v = f[fn](a)
    return round_to_f32_bits(v)


def entry(family, a_bits, b_bits, y_bits):
    fn = family.split("_")[0]
    with np.errstate(over="ignore"):
        host = int(np.array([_f64(y_bits)], np.float64).astype(np.float32).view(np.uint32)[0])
    cr = correctly_rounded(fn, a_bits, b_bits)
    e = {"fn": fn, "family": family, "a": f"0x{a_bits:08x}"}
    if fn in ("pow", "atan2"):
        e["b"] = f"0x{b_bits:08x}"
    e.update({"host_f64": f"0x{y_bits:016x}", "host_f32": f"0x{host:08x}", "cr_f32": f"0x{cr:08x}",
              "double_rounding": host != cr})
    return e


def glibc_version():
    return "-".join(platform.libc_ver())


def generate(exe, log=lambda s: None):
    rows = []
    for fn in ONE_ARGUMENT:
        r = mine(exe, "one", fn, 0, 1 << 32)
        log(f"{fn}: {len(r)}")
        rows += r
    for args in (("pow_srgb",), ("pow_burn",), ("pow_fit",) + POW_FIT_GRID, ("atan2", ATAN2_SEED, ATAN2_VECTORS)):
        r = mine(exe, *args)
        log(f"{args[0]}: {len(r)}")
        rows += r
    entries = [entry(*r) for r in rows]
    counts, flagged = {}, {}
    for e in entries:
        counts[e["family"]] = counts.get(e["family"], 0) + 1
        flagged[e["family"]] = flagged.get(e["family"], 0) + int(e["double_rounding"])
    header = {"glibc": glibc_version(), "margin_ulps": MARGIN, "mpmath_precision_bits": PRECISION,
              "one_argument": "every finite float32 input",
              "pow_srgb": "every positive finite a, b = (float)(1.0 / 2.4)",
              "pow_burn": "every positive finite a, b = 4.0f",
              "pow_fit_pairs": POW_FIT_GRID[0] * POW_FIT_GRID[1], "pow_fit_grid": list(POW_FIT_GRID),
              "atan2_seed": ATAN2_SEED, "atan2_pairs": 2 * ATAN2_VECTORS,
              "entries": counts, "double_rounding": flagged}
    return {"header": header, "entries": entries}


def dumps(fixture):
    lines = ["{", '"header": ' + json.dumps(fixture["header"], sort_keys=True) + ",", '"entries": [']
    lines += [json.dumps(e) + ("," if i + 1 < len(fixture["entries"]) else "") for i, e in enumerate(fixture["entries"])]
    lines += ["]", "}"]
    return "\n".join(lines) + "\n"


def main():
    if compiler() is None:
        sys.exit("make_cr_hard_cases: no g++")
    with tempfile.TemporaryDirectory() as tmp:
        fixture = generate(build_miner(tmp), log=lambda s: print(s, flush=True))
    os.makedirs(os.path.dirname(FIXTURE), exist_ok=True)
    with open(FIXTURE, "w") as f:
        f.write(dumps(fixture))
    print(f"wrote {FIXTURE}: {len(fixture['entries'])} entries, "
          f"{sum(e['double_rounding'] for e in fixture['entries'])} with double rounding")


if __name__ == "__main__":
    main()
