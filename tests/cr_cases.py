"""Shared by tests/test_cr_math_host.py and tests/test_gpu_cr_math.py: the hard-case fixture
tests/golden/cr_hard_cases.json (tools/make_cr_hard_cases.py), the input families of the cr_* call
sites restated in numpy, and the chunked, threaded host twin."""
import importlib.util
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "cr_hard_cases.json")
ONE_ARGUMENT = ["sin", "cos", "tan", "acos", "atan", "exp", "log", "log2"]
HOST_THREADS = 16          # a fixed pool, not the machine's CPU count

_cache = {}


def fixture():
    if "fixture" not in _cache:
        with open(FIXTURE) as f:
            _cache["fixture"] = json.load(f)
    return _cache["fixture"]


def entries(fn):
    """The fixture's entries of function `fn` as arrays: a, b (uint32 bits), y (uint64 bits), host, cr
    (uint32 bits), flag (bool)."""
    es = [e for e in fixture()["entries"] if e["fn"] == fn]
    col = lambda k, dt: np.array([int(e.get(k, "0x0"), 16) for e in es], dtype=dt)   # noqa: E731
    return {"a": col("a", np.uint32), "b": col("b", np.uint32), "y": col("host_f64", np.uint64),
            "host": col("host_f32", np.uint32), "cr": col("cr_f32", np.uint32),
            "flag": np.array([e["double_rounding"] for e in es], dtype=bool)}


def maker():
    """tools/make_cr_hard_cases.py as a module."""
    if "maker" not in _cache:
        spec = importlib.util.spec_from_file_location("make_cr_hard_cases",
                                                      os.path.join(ROOT, "tools", "make_cr_hard_cases.py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        _cache["maker"] = m
    return _cache["maker"]


def step_f64(y_bits, k):
    """float64 bit patterns moved by k ulps along the ordered doubles (cr_mine.cpp's step)."""
    i = y_bits.astype(np.uint64).view(np.int64)
    lo = np.int64(np.iinfo(np.int64).min)
    o = np.where(i < 0, lo - i, i) + np.int64(k)
    return np.where(o < 0, lo - o, o).view(np.float64)


def host_eval(ctl, fn, a, b=None, chunk=1 << 18):
    """ctl.host_math_eval over chunks in a pool of HOST_THREADS threads (ctypes releases the GIL)."""
    a = np.ascontiguousarray(a)
    n = a.size
    if n <= chunk:
        return ctl.host_math_eval(fn, a, b)
    out = np.empty(n, np.uint32)

    def run(s):
        out[s:s + chunk] = ctl.host_math_eval(fn, a[s:s + chunk], None if b is None else b[s:s + chunk])

    with ThreadPoolExecutor(HOST_THREADS) as pool:
        list(pool.map(run, range(0, n, chunk)))
    return out


def is_nan_bits(u):
    return (u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)


def differing(got, want):
    """Indices where two arrays of float32 bits differ, both-NaN counting as equal."""
    return np.flatnonzero((got != want) & ~(is_nan_bits(got) & is_nan_bits(want)))


# --- the generator of cr_mine.cpp (splitmix64, cube point normalised in fp32) ---------------------
def unit_vectors(seed, n, start=0):
    M = np.uint64(0xFFFFFFFFFFFFFFFF)
    with np.errstate(over="ignore"):
        i = np.arange(start, start + n, dtype=np.uint64)
        z = (np.uint64(seed) + (i + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)) & M
        z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & M
        z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & M
        h = z ^ (z >> np.uint64(31))
    f = np.float32
    v = [(((h >> np.uint64(21 * c)) & np.uint64(0x1fffff)).astype(np.float32) + f(0.5)) * f(1.0 / 1048576.0) - f(1.0)
         for c in range(3)]
    l = np.zeros(n, np.float32)
    for c in range(3):
        l = l + v[c] * v[c]
    l = np.sqrt(l)
    return np.stack([v[c] / l for c in range(3)], axis=1)


def atan2_pairs(seed, n_vectors):
    """(y, x) arguments of the two call-site families: (d.x, -d.z) and (d.y, d.x)."""
    d = unit_vectors(seed, n_vectors)
    return np.concatenate([d[:, 0], d[:, 1]]), np.concatenate([-d[:, 2], d[:, 0]])


def pow_fit_pairs(nx, nt):
    """(1 - sample_x, fit) of mf_sample_visible11 (ctl_bsdf.h) on an nx x nt grid, in fp32."""
    f = np.float32
    theta = f(1e-4) + (f(3.14159265358979) - f(1e-4)) * (np.arange(nt, dtype=np.float32) / f(nt - 1))
    fit = f(1) + theta * (f(-0.876) + theta * (f(0.4265) - f(0.0594) * theta))
    sx = f(1e-6) + (f(1.0) - f(1e-6)) * (np.arange(nx, dtype=np.float32) / f(nx))
    a = f(1) - sx
    return np.tile(a, nt), np.repeat(fit, nx)


# each argument of the special-value table
SPECIALS = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00800000, 0x80800000, 0x3f800000, 0xbf800000,
                     0x7f7fffff, 0xff7fffff, 0x7f800000, 0xff800000, 0x7fc00000], dtype=np.uint32)


def special_table():
    a, b = np.meshgrid(SPECIALS, SPECIALS, indexing="ij")
    return a.ravel().copy(), b.ravel().copy()
