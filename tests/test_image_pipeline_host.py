"""Image pipeline, host side (no GPU): the new C-ABI symbols and struct sizes, and
the host helpers (ctl_filter_evaluate, ctl_rgbe_encode / decode,
ctl_tonemap_constants) bit for bit against the numpy restatement in
image_pipeline_ref.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_pipeline_ref as ref  # noqa: E402

import cudatracerlib_amd._abi as abi  # noqa: E402

f32 = np.float32
NEW_SYMBOLS = ["ctl_image_pipeline", "ctl_image_luminance", "ctl_filter_evaluate", "ctl_rgbe_encode",
               "ctl_rgbe_decode", "ctl_tonemap_constants"]


def bits(x):
    return np.asarray(x, f32).view(np.uint32)


def test_symbols_and_struct_sizes():
    lib = C.CDLL(abi.LIB_PATH)
    bound = {n for n, _, _ in abi.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in bound, name
    assert C.sizeof(abi.ImageFilter) == 36
    assert C.sizeof(abi.Tonemap) == 8
    assert C.sizeof(abi.LuminanceInfo) == 28
    assert (abi.CTL_FILTER_BOX, abi.CTL_FILTER_GAUSSIAN, abi.CTL_FILTER_MITCHELL, abi.CTL_FILTER_LANCZOS,
            abi.CTL_FILTER_TRIANGLE, abi.CTL_FILTER_NLM, abi.CTL_NLM_DIRECT) == (1, 2, 3, 4, 5, 16, 1)
    assert abi.load().ctl_abi_version() == 4


# (type, non-default parameters)
FILTER_CASES = [
    (abi.CTL_FILTER_BOX, {}), (abi.CTL_FILTER_BOX, dict(x_width=0.5, y_width=3.25)),
    (abi.CTL_FILTER_GAUSSIAN, {}), (abi.CTL_FILTER_GAUSSIAN, dict(x_width=1.5, y_width=2.25, a=2.0)),
    (abi.CTL_FILTER_MITCHELL, {}), (abi.CTL_FILTER_MITCHELL, dict(x_width=1.5, y_width=2.25, a=0.0, b=0.5)),
    (abi.CTL_FILTER_LANCZOS, {}), (abi.CTL_FILTER_LANCZOS, dict(x_width=1.5, y_width=2.25, a=2.0)),
    (abi.CTL_FILTER_TRIANGLE, {}), (abi.CTL_FILTER_TRIANGLE, dict(x_width=1.5, y_width=2.25)),
]


@pytest.mark.parametrize("ftype,params", FILTER_CASES)
def test_filter_evaluate_matches_restatement(ctl, ftype, params):
    f = ctl.image_filter(ftype, **params)
    # |x| in [0, x_width], |y| in [0, y_width]: the integer distances a window holds, the ends, fractions
    xs = np.unique(np.concatenate([np.arange(0, int(f.x_width) + 1, dtype=f32), np.linspace(0, f.x_width, 9, dtype=f32),
                                   f32([1e-6, 2e-5])]))
    ys = np.unique(np.concatenate([np.arange(0, int(f.y_width) + 1, dtype=f32), np.linspace(0, f.y_width, 7, dtype=f32)]))
    X, Y = np.meshgrid(xs, ys)
    want = ref.filter_evaluate(f, X.reshape(-1), Y.reshape(-1))
    got = np.array([ctl.filter_evaluate(f, x, y) for x, y in zip(X.reshape(-1), Y.reshape(-1))], f32)
    assert np.array_equal(bits(got), bits(want))
    if ftype != abi.CTL_FILTER_GAUSSIAN or params:   # the reference's default alpha (-2) makes every weight 0
        assert (want != 0).any()


def test_filter_evaluate_refuses_other_types(ctl):
    with pytest.raises(ctl.CTLError, match="canonical"):
        ctl.filter_evaluate(ctl.image_filter(abi.CTL_FILTER_NLM), 0.0, 0.0)
    with pytest.raises(ctl.CTLError, match="canonical"):
        ctl.filter_evaluate(ctl.image_filter(7, 1.0, 1.0), 0.0, 0.0)


def rgbe_inputs():
    step = np.nextafter(f32(1.5), f32(2))
    rows = [
        (0, 0, 0), (1e-33, 1e-33, 1e-33), (1e-33, 0, 2e-32), (1e-32, 1e-32, 1e-32),
        (1, 1, 1), (0.5, 0.25, 0.125), (2, 4, 8), (1024, 1, 1.0 / 1024), (2.0 ** -20, 2.0 ** -21, 2.0 ** -30),
        # values straddling a step of the 8-bit mantissa (k / 256 of the leading power of two)
        (1.5, np.nextafter(f32(1.5), f32(0)), step), (255.0 / 256, np.nextafter(f32(255.0 / 256), f32(0)), 1),
        (np.nextafter(f32(2), f32(0)), 1.0 + 1.0 / 128, np.nextafter(f32(1.0 + 1.0 / 128), f32(0))),
        (0.3, 0.6, 0.9), (1e30, 5e29, 1e10), (1e30, 1e30, 1e30), (3.0e38, 1.0, 2.0),
        (-1.0, 0.5, 0.25), (0.5, -0.25, -1e30), (-1, -2, -3),
        (np.nan, 0.5, 0.25), (0.5, np.nan, 0.25), (0.5, 0.25, np.nan), (np.inf, 1.0, 2.0),
    ]
    rng = np.random.default_rng(3)
    rnd = (rng.random((64, 3)) * 10.0 ** rng.integers(-12, 12, (64, 1))).astype(f32)
    return np.concatenate([np.array(rows, f32), rnd])


def test_rgbe_encode_decode_match_restatement(ctl):
    rgb = rgbe_inputs()
    want = ref.rgbe_encode(rgb)
    got = np.array([ctl.rgbe_encode(c) for c in rgb], np.uint32)
    assert np.array_equal(got, want), [(list(c), hex(g), hex(w)) for c, g, w in zip(rgb, got, want) if g != w]
    assert got[0] == 0 and got[1] == 0                        # zeros, and a maximum below 1e-32
    assert got[4] == (128 | 128 << 8 | 128 << 16 | 129 << 24)  # 1 = 0.5 * 2^1 -> mantissa 128, exponent 1 + 128
    assert got[16] >> 24 != 0 and got[16] & 0xff == 0         # a negative component saturates to 0
    assert got[19] & 0xff == 0                                # a NaN component gives byte 0
    words = np.concatenate([got, np.array([0x00ffffff, 0x01ffffff, 0x0affffff, 0xff010203, 0x80ff0001], np.uint32)])
    dec_want = ref.rgbe_decode(words)
    dec_got = np.stack([ctl.rgbe_decode(int(v)) for v in words])
    assert np.array_equal(bits(dec_got), bits(dec_want))
    # a decoded colour encodes to its own record (away from the 1e-32 cut and the exponent's wrap)
    again = np.array([ctl.rgbe_encode(c) for c in dec_got[:len(got)]], np.uint32)
    keep = (got >> 24 != 0) & ((got & 0xffffff) != 0) & np.isfinite(rgb).all(1) & (rgb.max(1) < 1e38) & (rgb.max(1) > 1e-30)
    assert np.array_equal(again[keep], got[keep])


@pytest.mark.parametrize("key,burn", [(0.18, 0.0), (0.18, 0.5), (0.5, 0.7), (0.18, 1.0)])
@pytest.mark.parametrize("avg_log_lum,max_lum", [(0.37, 12.5), (2.3e-5, 0.0), (41.0, 980.0)])
def test_tonemap_constants_match_restatement(ctl, key, burn, avg_log_lum, max_lum):
    got = ctl.tonemap_constants(ctl.Tonemap(key, burn), avg_log_lum, max_lum)
    want = ref.tonemap_constants(key, burn, avg_log_lum, max_lum)
    assert np.array_equal(bits(got), bits(want))
    if max_lum == 0.0:
        assert np.isinf(got[1])          # Lwhite = 0: 1 / 0
