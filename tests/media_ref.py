"""The five medium operations in float64 numpy, written from the formulas (a slab test of the unit cube in
volume space, Beer-Lambert transmittance, the balance-heuristic distance sample over the RGB channels, the
isotropic and the Henyey-Greenstein phase functions), vectorised over queries.

A volume is a dict: w2v (4x4 float64, world to volume, affine), sig_a, sig_s (3,), phase ("isotropic" or
"hg"), g.  Besides each op's outputs the functions return what a test needs to judge a comparison with
fp32: which slab axis decided a bound and how far a branch's operands lie from its threshold."""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
EPSILON = 1e-6            # below this |g| the HG sample is the isotropic cosine
INV_FOURPI = 1.0 / (4.0 * np.pi)


def to_volume(V, ori, dir_):
    M = np.asarray(V["w2v"], np.float64)
    o = ori @ M[:3, :3].T + M[:3, 3]
    d = dir_ @ M[:3, :3].T
    return o, d


def intersect(V, ori, dir_, tmin, tmax):
    """hit, t0, t1, and per bound the |d| of the axis that set it (inf where tmin / tmax set it)."""
    o, d = to_volume(V, np.asarray(ori, np.float64), np.asarray(dir_, np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        ta, tb = (0.0 - o) / d, (1.0 - o) / d
    near, far = np.minimum(ta, tb), np.maximum(ta, tb)
    lo_axis, hi_axis = near.argmax(axis=1), far.argmin(axis=1)
    lo_box, hi_box = near.max(axis=1), far.min(axis=1)
    tmin, tmax = np.asarray(tmin, np.float64), np.asarray(tmax, np.float64)
    lo, hi = np.maximum(lo_box, tmin), np.minimum(hi_box, tmax)
    ad = np.abs(d)
    rows = np.arange(ad.shape[0])
    d_lo = np.where(lo_box > tmin, ad[rows, lo_axis], np.inf)
    d_hi = np.where(hi_box < tmax, ad[rows, hi_axis], np.inf)
    hit = (hi > lo) & (hi > 0)
    return dict(hit=hit, t0=lo, t1=hi, d_lo=d_lo, d_hi=d_hi, o=o, d=d)


def transmittance(V, ori, dir_, tmin, tmax):
    r = intersect(V, ori, dir_, tmin, tmax)
    sig_t = np.asarray(V["sig_a"], np.float64) + np.asarray(V["sig_s"], np.float64)
    length = np.where(r["hit"], np.linalg.norm(np.asarray(dir_, np.float64), axis=1) * (r["t1"] - r["t0"]), 0.0)
    r["length"] = length
    r["transmittance"] = np.exp(-length[:, None] * sig_t[None, :])
    return r


def sampling_weight(V):
    sig_s = np.asarray(V["sig_s"], np.float64)
    sig_t = np.asarray(V["sig_a"], np.float64) + sig_s
    w = -1.0
    for i in range(3):
        if sig_t[i] != 0 and sig_s[i] / sig_t[i] > w:
            w = sig_s[i] / sig_t[i]
    return max(w, 0.5) if w > 0 else w


def sample_distance(V, ori, dir_, tmin, tmax, u):
    ori, dir_ = np.asarray(ori, np.float64), np.asarray(dir_, np.float64)
    tmin, tmax, u = (np.asarray(a, np.float64) for a in (tmin, tmax, u))
    sig_a, sig_s = np.asarray(V["sig_a"], np.float64), np.asarray(V["sig_s"], np.float64)
    sig_t = sig_a + sig_s
    w = sampling_weight(V)
    n = u.shape[0]
    tried = u < w
    v = np.where(tried, u / (w if w > 0 else 1.0), 0.0) * 3.0
    channel = np.minimum(v.astype(np.int64), 2)
    u1 = v - channel
    with np.errstate(divide="ignore", invalid="ignore"):
        sd = np.where(tried, -np.log1p(-u1) / sig_t[channel], np.inf)
    span = tmax - tmin
    inside = sd < span
    dist = np.where(inside, sd, span)
    t = np.where(inside, tmin + dist, 0.0)
    p = np.where(inside[:, None], ori + t[:, None] * dir_, 0.0)
    success = inside & np.any(p != ori, axis=1)
    tr = np.exp(-dist[:, None] * sig_t[None, :])
    pdf_failure = w * tr.mean(axis=1) + (1.0 - w)
    pdf_success = w * (tr * sig_t[None, :]).mean(axis=1)
    tr_max = tr.max(axis=1)
    flushed = tr_max < 1e-8
    tr_out = np.where(flushed[:, None], 0.0, tr)
    return dict(success=success, inside=inside, t=t, p=p, transmittance=tr_out, pdf_success=pdf_success,
                pdf_failure=pdf_failure, sigma_a=np.where(inside[:, None], sig_a, 0.0),
                sigma_s=np.where(inside[:, None], sig_s, 0.0), weight=w, channel=channel, u1=u1, sd=sd, dist=dist,
                span=span, tr_max=tr_max, tried=tried, v=v, sig_t=sig_t)


def inside(V, p):
    M = np.asarray(V["w2v"], np.float64)
    pl = np.asarray(p, np.float64) @ M[:3, :3].T + M[:3, 3]
    return np.all((pl >= 0) & (pl <= 1), axis=1), pl


def hg(g, cos_wi_wo):
    temp = 1.0 + g * g + 2.0 * g * cos_wi_wo
    return INV_FOURPI * (1.0 - g * g) / (temp * np.sqrt(temp)), temp


def phase_value(V, wi, wo):
    """The phase function alone (no box): value and, for HG, the denominator's base."""
    wi, wo = np.asarray(wi, np.float64), np.asarray(wo, np.float64)
    if V["phase"] == "hg":
        return hg(float(V["g"]), np.sum(wi * wo, axis=1))
    return np.full(wi.shape[0], INV_FOURPI), np.ones(wi.shape[0])


def phase_eval(V, p, wi, wo):
    ins, pl = inside(V, p)
    val, temp = phase_value(V, wi, wo)
    scatters = np.mean(np.asarray(V["sig_s"], np.float64)) != 0
    return dict(value=np.where(ins & scatters, val, 0.0), inside=ins, pl=pl, temp=temp)


def frame(n):
    """The orthonormal basis (s, t, n) the reference's Frame(n) builds: t in the plane of n's larger of
    x / y and z, s = t x n."""
    n = np.asarray(n, np.float64)
    big_x = np.abs(n[:, 0]) > np.abs(n[:, 1])
    z = np.zeros(n.shape[0])
    with np.errstate(divide="ignore", invalid="ignore"):
        tx = np.stack([n[:, 2], z, -n[:, 0]], axis=1) / np.sqrt(n[:, 0] ** 2 + n[:, 2] ** 2)[:, None]
        ty = np.stack([z, n[:, 2], -n[:, 1]], axis=1) / np.sqrt(n[:, 1] ** 2 + n[:, 2] ** 2)[:, None]
    t = np.where(big_x[:, None], tx, ty)
    s = np.cross(t, n)
    s /= np.linalg.norm(s, axis=1)[:, None]
    return s, t, n


def phase_sample(V, wi, u):
    """wo, cos_theta, sin_theta of the sample.  Isotropic: z = 1 - 2 u.y about the world z axis, phi =
    2 pi u.x.  HG: cos_theta from u.x about -wi (the isotropic cosine below EPSILON), phi = 2 pi u.y."""
    wi, u = np.asarray(wi, np.float64), np.asarray(u, np.float64)
    if V["phase"] == "hg":
        g = float(V["g"])
        if abs(g) < EPSILON:
            c = 1.0 - 2.0 * u[:, 0]
        else:
            sq = (1.0 - g * g) / (1.0 - g + 2.0 * g * u[:, 0])
            c = (1.0 + g * g - sq * sq) / (2.0 * g)
        s_ = np.sqrt(np.maximum(0.0, 1.0 - c * c))
        phi = 2.0 * np.pi * u[:, 1]
        fs, ft, fn = frame(-wi)
        wo = fs * (s_ * np.cos(phi))[:, None] + ft * (s_ * np.sin(phi))[:, None] + fn * c[:, None]
        return dict(wo=wo, cos_theta=c, sin_theta=s_, xy_gap=np.abs(np.abs(wi[:, 0]) - np.abs(wi[:, 1])))
    c = 1.0 - 2.0 * u[:, 1]
    s_ = np.sqrt(np.maximum(0.0, 1.0 - c * c))
    phi = 2.0 * np.pi * u[:, 0]
    wo = np.stack([s_ * np.cos(phi), s_ * np.sin(phi), c], axis=1)
    return dict(wo=wo, cos_theta=c, sin_theta=s_, xy_gap=np.full(wi.shape[0], np.inf))
