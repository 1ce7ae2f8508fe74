#!/usr/bin/env python3
"""Every one of the 2^32 float32 bit patterns through each one-argument cr_* function: the HIP entry
ctl_math_eval against its host twin ctl_host_math_eval, bit for bit (two NaNs count as equal).

A tool, not a test: a few minutes on one MI355X and 16 host threads.  Inputs are made on the device
from an integer range, in chunks of 2^26; the host side runs in at most 16 threads.  Writes, per
function, the number of differing inputs and the first few of them, with the ROCm and glibc versions.

    python tools/cr_exhaustive.py --out profiles/cr_exhaustive.json
"""
import argparse
import json
import os
import platform
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FUNCTIONS = ["sin", "cos", "tan", "acos", "atan", "exp", "log", "log2"]
CHUNK = 1 << 26
PIECE = 1 << 20
THREADS = 16
KEEP = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cr_exhaustive.json"))
    ap.add_argument("--functions", nargs="*", default=FUNCTIONS)
    args = ap.parse_args()

    import torch

    import cudatracerlib_amd as ctl

    dev = torch.device("cuda:0")
    t = ctl.Tracer(0)
    out = torch.zeros(CHUNK, dtype=torch.int32, device=dev)
    result = {"rocm": torch.version.hip, "glibc": "-".join(platform.libc_ver()), "device": torch.cuda.get_device_name(0),
              "inputs_per_function": 1 << 32, "nan_rule": "two NaNs count as equal", "functions": {}}
    pool = ThreadPoolExecutor(THREADS)
    for fn in args.functions:
        t0 = time.time()
        differing, first = 0, []
        for start in range(0, 1 << 32, CHUNK):
            x = torch.arange(start, start + CHUNK, dtype=torch.int64, device=dev).to(torch.int32)   # wraps to the bit pattern
            t.math_eval(fn, CHUNK, x.data_ptr(), 0, out.data_ptr())
            torch.cuda.synchronize()
            got = out.cpu().numpy().view(np.uint32)

            def piece(s, start=start, got=got):
                a = np.arange(start + s, start + s + PIECE, dtype=np.uint64).astype(np.uint32)
                want = ctl.host_math_eval(fn, a)
                g = got[s:s + PIECE]
                nan = lambda u: (u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)   # noqa: E731
                bad = np.flatnonzero((g != want) & ~(nan(g) & nan(want)))
                return [(int(a[i]), int(g[i]), int(want[i])) for i in bad]

            for bad in pool.map(piece, range(0, CHUNK, PIECE)):
                differing += len(bad)
                first += bad[:max(0, KEEP - len(first))]
        result["functions"][fn] = {"differing": differing, "seconds": round(time.time() - t0, 1),
                                   "first": [{"x": f"0x{x:08x}", "device": f"0x{g:08x}", "host": f"0x{w:08x}"}
                                             for x, g, w in first]}
        print(f"{fn}: {differing} of 2^32 inputs differ ({time.time() - t0:.0f} s)", flush=True)
    t.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
