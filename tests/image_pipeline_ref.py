"""numpy fp32 restatement of the image pipeline (not a test): the arithmetic of
cudatracerlib_amd/csrc/ctl_image.h and the kernels of csrc/device/pipeline.hip
in the reference's operation order (Kernel/ImagePipeline, Math/Spectrum,
SceneTypes/Filter.h, Engine/Image.cu), every intermediate np.float32.

exp / log / pow / sin go through Python's math module (the C library's double
functions) on the float64 value and are rounded to fp32, as the library's
cr_* functions do.  Sums are taken in the order the kernels document.
Vectorised over pixels; loops run over filter offsets."""
import math

import numpy as np

f32 = np.float32
FILTER_BOX, FILTER_GAUSSIAN, FILTER_MITCHELL, FILTER_LANCZOS, FILTER_TRIANGLE, FILTER_NLM = 1, 2, 3, 4, 5, 16
NLM_R, NLM_F = 6, 3
PI = f32(3.14159265358979)

_ERR = dict(over="ignore", under="ignore", invalid="ignore", divide="ignore")


def _exp(v):
    if v != v:
        return v
    try:
        return math.exp(v)
    except OverflowError:
        return math.inf


def _log(v):
    if v != v or v < 0:
        return math.nan
    if v == 0:
        return -math.inf
    return math.log(v)


def _pow(a, b):
    try:
        return math.pow(a, b)
    except OverflowError:
        return math.inf
    except ValueError:
        return math.nan


def _map(fn, x, *rest):
    """fn on the float64 value of every fp32 element, rounded to fp32"""
    x = np.asarray(x, f32)
    flat = x.reshape(-1).astype(np.float64).tolist()
    with np.errstate(**_ERR):
        return np.array([fn(v, *rest) for v in flat], np.float64).astype(f32).reshape(x.shape)


def cr_exp(x): return _map(_exp, x)
def cr_log(x): return _map(_log, x)
def cr_sin(x): return _map(lambda v: math.sin(v) if math.isfinite(v) else math.nan, x)
def cr_pow(x, b): return _map(_pow, x, float(f32(b)))


def tmax(a, b): return np.where(a > b, a, b).astype(f32)      # (a > b) ? a : b
def tmin(a, b): return np.where(a < b, a, b).astype(f32)      # (a < b) ? a : b


# ---- sRGB / RGBCOL ---------------------------------------------------------

def to_srgb(v):
    v = np.asarray(v, f32)
    lin = v <= f32(0.0031308)
    out = f32(12.92) * v
    if (~lin).any():
        out = out.copy()
        out[~lin] = f32(1.055) * cr_pow(v[~lin], f32(1.0 / 2.4)) - f32(0.055)
    return out.astype(f32)


def to_u8(x):
    with np.errstate(**_ERR):
        c = tmin(tmax(np.asarray(x, f32), f32(0)), f32(1)) * f32(255)
        return c.astype(np.uint32) & np.uint32(0xff)


def to_rgbcol(c):
    b = to_u8(c)
    return (b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16) | np.uint32(255 << 24)).astype(np.uint32)


def from_rgbcol(w):
    w = np.asarray(w, np.uint32)
    return np.stack([(w >> s & 0xff).astype(f32) / f32(255) for s in (0, 8, 16)], -1).astype(f32)


def gamma_correct(c):
    return to_rgbcol(to_srgb(c))


def pixel_to_spectrum(fb, splat):
    fb = np.asarray(fb, f32).reshape(-1, 7)
    weight = np.where(fb[:, 6] != 0, fb[:, 6], f32(1)).astype(f32)
    recip = f32(1) / weight
    return (fb[:, 0:3] * recip[:, None] + fb[:, 3:6] * f32(splat)).astype(f32)


# ---- RGBE ------------------------------------------------------------------

def _rgbe_byte(v):
    with np.errstate(**_ERR):
        t = np.where(v > 0, np.where(v >= 255, f32(255), v), f32(0))   # NaN and negatives -> 0
        return t.astype(np.uint32)


def rgbe_encode(c):
    c = np.asarray(c, f32).reshape(-1, 3)
    with np.errstate(**_ERR):
        max_ = tmax(tmax(c[:, 0], c[:, 1]), c[:, 2])
        zero = max_.astype(np.float64) < 1e-32
        finite = np.isfinite(max_)
        frac, e = np.frexp(np.where(finite, max_, f32(1)))
        frac = np.where(finite, frac, max_).astype(f32)
        e = np.where(finite, e, 0)
        m = (frac * f32(256) / max_).astype(f32)
        word = (_rgbe_byte(c[:, 0] * m) | (_rgbe_byte(c[:, 1] * m) << 8) | (_rgbe_byte(c[:, 2] * m) << 16) |
                (((e + 128) & 0xff).astype(np.uint32) << 24))
    return np.where(zero, 0, word).astype(np.uint32)


def rgbe_decode(w):
    w = np.asarray(w, np.uint32).reshape(-1)
    e = (w >> 24).astype(np.int32)
    exp = np.ldexp(f32(1), e - 136).astype(f32)
    c = np.stack([(w >> s & 0xff).astype(f32) * exp for s in (0, 8, 16)], -1).astype(f32)
    return np.where((e != 0)[:, None], c, f32(0)).astype(f32)


# ---- colour spaces ---------------------------------------------------------

def clamp_ref(v, lo, hi): return tmin(tmax(v, f32(lo)), f32(hi))


def to_xyz(s):
    x = s[:, 0] * f32(0.412453) + s[:, 1] * f32(0.357580) + s[:, 2] * f32(0.180423)
    y = s[:, 0] * f32(0.212671) + s[:, 1] * f32(0.715160) + s[:, 2] * f32(0.072169)
    z = s[:, 0] * f32(0.019334) + s[:, 1] * f32(0.119193) + s[:, 2] * f32(0.950227)
    return x, y, z


def from_xyz(x, y, z):
    return np.stack([f32(3.240479) * x + f32(-1.537150) * y + f32(-0.498535) * z,
                     f32(-0.969256) * x + f32(1.875991) * y + f32(0.041556) * z,
                     f32(0.055648) * x + f32(-0.204043) * y + f32(1.057311) * z], -1).astype(f32)


def get_luminance(s):
    return (s[:, 0] * f32(0.212671) + s[:, 1] * f32(0.715160) + s[:, 2] * f32(0.072169)).astype(f32)


def to_Yxy(c):
    X, Y, Z = to_xyz(c)
    s = clamp_ref(X + Y + Z, 0.001, 100000.0)
    return Y, X / s, Y / s


def from_Yxy(_Y, x, y):
    X = _Y / clamp_ref(y, 0.001, 100000.0) * x
    Z = _Y / clamp_ref(y, 0.001, 100000.0) * (f32(1) - x - y)
    return from_xyz(X, _Y, Z)


# ---- tone map --------------------------------------------------------------

def tonemap_constants(key, burn_in, avg_log_lum, max_lum):
    with np.errstate(**_ERR):
        scale = f32(key) / f32(avg_log_lum)
        Lwhite = f32(max_lum) * scale
        burn = tmin(f32(1), tmax(f32(1e-8), f32(1) - f32(burn_in)))
        inv_wp2 = f32(1) / (Lwhite * Lwhite * cr_pow(burn, 4.0))
    return f32(scale), f32(inv_wp2)


def reinhard(rgbe, scale, inv_wp2):
    with np.errstate(**_ERR):
        Y, x, y = to_Yxy(rgbe_decode(rgbe))
        Lp = f32(scale) * Y
        Y = Lp * (f32(1) + Lp * f32(inv_wp2)) / (f32(1) + Lp)
        return to_rgbcol(from_Yxy(Y, x, y))


# ---- luminance -------------------------------------------------------------

def _block_combine(s):
    """s: (..., 256) per-lane values -> the workgroup total: xor butterfly 32 .. 1
    inside each wave of 64, then the four wave sums in wave order."""
    v = s.reshape(s.shape[:-1] + (4, 64)).astype(f32)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., lane ^ off]).astype(f32)
    wv = v[..., 0]
    return (((wv[..., 0] + wv[..., 1]) + wv[..., 2]) + wv[..., 3]).astype(f32)


def _strided_lane_sums(terms, groups):
    """terms: (n,) -> (groups, 256): lane t of group g adds elements
    g*256 + t + j*groups*256, j = 0, 1, ..., in that order"""
    n = terms.shape[0]
    stride = groups * 256
    J = (n + stride - 1) // stride
    pad = np.zeros(J * stride, f32)
    pad[:n] = terms
    valid = np.zeros(J * stride, bool)
    valid[:n] = True
    pad, valid = pad.reshape(J, groups, 256), valid.reshape(J, groups, 256)
    s = np.zeros((groups, 256), f32)
    for j in range(J):
        s = np.where(valid[j], (s + pad[j]).astype(f32), s)
    return s, J


def ordered_sum(terms):
    """The device's documented order; returns (sum, depth of the longest chain of additions)."""
    terms = np.asarray(terms, f32).reshape(-1)
    n = terms.shape[0]
    G = min((n + 255) // 256, 1024)
    lanes, J = _strided_lane_sums(terms, G)
    partial = _block_combine(lanes)                      # (G,)
    lanes2, J2 = _strided_lane_sums(partial, 1)
    return f32(_block_combine(lanes2)[0]), J + 9 + J2 + 9


def luminance_terms(rgbe):
    L = rgbe_decode(rgbe)
    Y = get_luminance(L)
    return L, Y, cr_log(f32(2.3e-5) + Y)


def luminance(rgbe, w, h):
    """ctl_image_luminance: dict of avg_color[3], min_lum, max_lum, avg_lum, avg_log_lum (fp32)"""
    L, Y, lg = luminance_terms(rgbe)
    n = f32(np.uint32(w * h))
    nc = f32(w) * f32(h)
    recip = f32(1) / nc
    return dict(avg_color=np.array([ordered_sum(L[:, i])[0] * recip for i in range(3)], f32),
                min_lum=f32(Y.min()), max_lum=f32(max(f32(0), Y.max())), avg_lum=f32(ordered_sum(Y)[0] / n),
                avg_log_lum=f32(cr_exp(ordered_sum(lg)[0] / n)))


# ---- canonical filters -----------------------------------------------------

def mitchell_1d(B, C, x):
    B, C = f32(B), f32(C)
    x = np.abs(f32(2) * np.asarray(x, f32))
    hi = ((-B - f32(6) * C) * x * x * x + (f32(6) * B + f32(30) * C) * x * x + (f32(-12) * B - f32(48) * C) * x +
          (f32(8) * B + f32(24) * C)) * (f32(1) / f32(6))
    lo = ((f32(12) - f32(9) * B - f32(6) * C) * x * x * x + (f32(-18) + f32(12) * B + f32(6) * C) * x * x +
          (f32(6) - f32(2) * B)) * (f32(1) / f32(6))
    return np.where(x > f32(1), hi, lo).astype(f32)


def lanczos_sinc_1d(tau, x):
    tau = f32(tau)
    x = np.abs(np.asarray(x, f32))
    with np.errstate(**_ERR):
        xp = x * PI
        sinc = cr_sin(xp) / xp
        lanczos = cr_sin(xp * tau) / (xp * tau)
        r = (sinc * lanczos).astype(f32)
    r = np.where(x.astype(np.float64) > 1.0, f32(0), r)
    return np.where(x.astype(np.float64) < 1e-5, f32(1), r).astype(f32)


def filter_factor(f, d, axis):
    d = np.asarray(d, f32)
    width = f32(f.y_width if axis else f.x_width)
    if f.type == FILTER_GAUSSIAN:
        alpha = f32(f.a)
        expv = cr_exp(-alpha * width * width)
        return tmax(f32(0), cr_exp(-alpha * d * d) - expv)
    if f.type == FILTER_MITCHELL:
        return mitchell_1d(f.a, f.b, d * (f32(1) / width))
    if f.type == FILTER_LANCZOS:
        return lanczos_sinc_1d(f.a, d * (f32(1) / width))
    if f.type == FILTER_TRIANGLE:
        return tmax(f32(0), width - np.abs(d))
    return np.ones(d.shape, f32)


def filter_evaluate(f, x, y):
    if f.type == FILTER_BOX:
        return np.ones(np.broadcast(np.asarray(x), np.asarray(y)).shape, f32)
    with np.errstate(**_ERR):
        return (filter_factor(f, x, 0) * filter_factor(f, y, 1)).astype(f32)


def canonical_filter(fb, w, h, splat, f):
    """CanonicalFilter's evalFilter for every pixel -> RGBE words (rows outer, columns inner)"""
    S = pixel_to_spectrum(fb, splat).reshape(h, w, 3)
    ys, xs = np.mgrid[0:h, 0:w]
    xw, yw = f32(f.x_width), f32(f.y_width)
    x0 = np.maximum(0, np.ceil(xs.astype(f32) - xw)).astype(np.int64)
    x1 = np.minimum(w - 1, np.floor(xs.astype(f32) + xw)).astype(np.int64)
    y0 = np.maximum(0, np.ceil(ys.astype(f32) - yw)).astype(np.int64)
    y1 = np.minimum(h - 1, np.floor(ys.astype(f32) + yw)).astype(np.int64)
    rx, ry = min(int(math.floor(xw)) + 1, w - 1), min(int(math.floor(yw)) + 1, h - 1)
    acc = np.zeros((h, w, 3), f32)
    accw = np.zeros((h, w), f32)
    with np.errstate(**_ERR):
        for dy in range(-ry, ry + 1):
            for dx in range(-rx, rx + 1):
                x, y = xs + dx, ys + dy
                m = (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1)
                if not m.any():
                    continue
                wt = filter_evaluate(f, f32(abs(dx)), f32(abs(dy))).reshape(())
                tap = S[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)]
                acc = np.where(m[..., None], (acc + tap * wt).astype(f32), acc)
                accw = np.where(m, (accw + wt).astype(f32), accw)
        recip = f32(1) / accw
        res = (acc * recip[..., None]).astype(f32)
    return rgbe_encode(res.reshape(-1, 3))


# ---- non-local means -------------------------------------------------------

def nlm_variance(var, sigma2_scale):
    """var: (n, 11) float32 view of ctl_pixel_variance records -> half-rounded variance * sigma2Scale"""
    var = np.asarray(var, f32).reshape(-1, 11)
    sum_x, sum_x2 = var[:, 8], var[:, 9]
    with np.errstate(**_ERR):
        N = var[:, 10].view(np.int32).astype(f32)
        invN = f32(1) / N
        v = ((sum_x2 - (sum_x * sum_x) * invN) * invN).astype(f32)
        return (v.astype(np.float16).astype(f32) * f32(sigma2_scale)).astype(f32)


def nlm_cached(fb, splat):
    """copyToCached + loadFromShared: the colours the filter sees"""
    return rgbe_decode(rgbe_encode(pixel_to_spectrum(fb, splat)))


def nlm_weights(fb, var, w, h, splat, k, sigma2_scale):
    """computeWeights: (h*w, 169) weights, index (yo + 6) * 13 + (xo + 6); entries whose q lies
    outside the image stay 0 (ClearBuffer)"""
    R, F, P = NLM_R, NLM_F, NLM_R + NLM_F
    k = f32(k)
    C = np.zeros((h + 2 * P, w + 2 * P, 3), f32)
    V = np.zeros((h + 2 * P, w + 2 * P), f32)
    I = np.zeros((h + 2 * P, w + 2 * P), bool)
    C[P:P + h, P:P + w] = nlm_cached(fb, splat).reshape(h, w, 3)
    V[P:P + h, P:P + w] = nlm_variance(var, sigma2_scale).reshape(h, w)
    I[P:P + h, P:P + w] = True
    out = np.zeros((h * w, 169), f32)

    def win(a, oy, ox, ny, nx):   # a[y + oy, x + ox] for y < ny, x < nx in padded coordinates
        return a[oy:oy + ny, ox:ox + nx]

    th, tw = h + 2 * F, w + 2 * F            # positions a = p + delta: [-F, h + F) x [-F, w + F)
    with np.errstate(**_ERR):
        for xo in range(-R, R + 1):
            for yo in range(-R, R + 1):
                cp, cq = win(C, P - F, P - F, th, tw), win(C, P - F + yo, P - F + xo, th, tw)
                vp, vq = win(V, P - F, P - F, th, tw), win(V, P - F + yo, P - F + xo, th, tw)
                ok = win(I, P - F, P - F, th, tw) & win(I, P - F + yo, P - F + xo, th, tw)
                sq = ((cp - cq) * (cp - cq)).astype(f32)
                s = np.zeros((th, tw), f32)
                for i in range(3):
                    s = (s + sq[..., i]).astype(f32)
                u = s * (f32(1) / f32(3))
                term = ((u - (vp + tmin(vp, vq))) / (f32(1e-10) + k * k * (vp + vq))).astype(f32)
                d = np.zeros((h, w), f32)
                cnt = np.zeros((h, w), f32)
                for x in range(-F, F + 1):
                    for y in range(-F, F + 1):
                        m = ok[F + y:F + y + h, F + x:F + x + w]
                        d = np.where(m, (d + term[F + y:F + y + h, F + x:F + x + w]).astype(f32), d)
                        cnt = cnt + m
                dr = np.where(cnt != 0, d / cnt.astype(f32), f32(0)).astype(f32)
                we = cr_exp(-np.fmax(f32(0), dr))
                we = np.where(we < f32(0.05), f32(0), we).astype(f32)
                qin = win(I, P + yo, P + xo, h, w)
                out[:, (yo + R) * 13 + (xo + R)] = np.where(qin, we, f32(0)).reshape(-1)
    return out


def nlm_apply(fb, weights, w, h, splat):
    """applyWeights -> RGBE words"""
    R = NLM_R
    col = nlm_cached(fb, splat).reshape(h, w, 3)
    C = np.zeros((h + 2 * R, w + 2 * R, 3), f32)
    I = np.zeros((h + 2 * R, w + 2 * R), bool)
    C[R:R + h, R:R + w] = col
    I[R:R + h, R:R + w] = True
    c_hat = np.zeros((h, w, 3), f32)
    C_p = np.zeros((h, w), f32)
    with np.errstate(**_ERR):
        for xo in range(-R, R + 1):
            for yo in range(-R, R + 1):
                we = weights[:, (yo + R) * 13 + (xo + R)].reshape(h, w)
                m = I[R + yo:R + yo + h, R + xo:R + xo + w] & ~np.isnan(we)
                cq = C[R + yo:R + yo + h, R + xo:R + xo + w]
                C_p = np.where(m, (C_p + we).astype(f32), C_p)
                c_hat = np.where(m[..., None], (c_hat + cq * we[..., None]).astype(f32), c_hat)
        recip = f32(1) / C_p
        res = np.where((C_p > f32(1e-4))[..., None], (c_hat * recip[..., None]).astype(f32), col)
    return rgbe_encode(res.reshape(-1, 3)), C_p


def nlm_check_non_vacuous(fb, weights, filtered, C_p, w, h, splat):
    """The input exercises the filter: thresholded and partial weights, a changed image, few fallbacks."""
    R = NLM_R
    ys, xs = np.mgrid[0:h, 0:w]
    inside = np.zeros((h * w, 169), bool)
    for xo in range(-R, R + 1):
        for yo in range(-R, R + 1):
            inside[:, (yo + R) * 13 + (xo + R)] = ((xs + xo >= 0) & (xs + xo < w) & (ys + yo >= 0) &
                                                   (ys + yo < h)).reshape(-1)
    wi = weights[inside]
    assert (wi == 0).sum() > 0, "no weight thresholded to 0"
    assert ((wi > f32(0.05)) & (wi < 1)).sum() > 0, "no weight in (0.05, 1)"
    own = rgbe_encode(pixel_to_spectrum(fb, splat))
    assert (filtered != own).sum() > (w * h) // 2, "the filter leaves most pixels unchanged"
    assert (C_p <= f32(1e-4)).sum() * 100 < w * h, "too many pixels take the C_p fallback"


# ---- applyImagePipeline ----------------------------------------------------

def finish(filtered, w, h, tonemap):
    """filtered RGBE -> RGBA: copyFilteredToOutput, or tone map + applyGammaCorrectureToOutput"""
    if tonemap is None:
        return gamma_correct(rgbe_decode(filtered))
    info = luminance(filtered, w, h)
    scale, inv = tonemap_constants(tonemap[0], tonemap[1], info["avg_log_lum"], info["max_lum"])
    return gamma_correct(from_rgbcol(reinhard(filtered, scale, inv)))


def resolve(fb, splat):
    """copySamplesToOutput"""
    return gamma_correct(pixel_to_spectrum(fb, splat))
