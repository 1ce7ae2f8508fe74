"""A float64 microfacet reference for the rough dielectric and the rough conductor, written from the
literature and vectorised with numpy.  It shares no code with ctl_bsdf.h or the oracle headers.

  Walter, Marschner, Li, Torrance 2007, "Microfacet Models for Refraction through Rough Surfaces":
    eq. 8   |dw_h / dw_o| = 1 / (4 |o.h|)                            reflection Jacobian
    eq. 16  h_t = -(n_i i + n_o o) / |n_i i + n_o o|                 refraction half vector
    eq. 17  |dw_h / dw_o| = n_o^2 |o.h| / (n_i (i.h) + n_o (o.h))^2  refraction Jacobian
    eq. 20  f_r = F G D / (4 |i.n| |o.n|)
    eq. 21  f_t = |i.h| |o.h| / (|i.n| |o.n|) * n_o^2 (1 - F) G D / (n_i (i.h) + n_o (o.h))^2
    eq. 23  G1(v, m) = chi+((v.m) / (v.n)) * smith(v)
    eq. 27  the rational fit of Beckmann's Smith G1
  Heitz 2014, "Understanding the Masking-Shadowing Function in Microfacet-Based BRDFs":
    the anisotropic D, Lambda and the density of visible normals
    D_wi(m) = G1(wi, m) |wi.m| D(m) / |wi.n|.

Conventions of the product that the reference adopts (they are conventions, not arithmetic):
  * the local frame, n = (0, 0, 1); wi is the side the query comes from, wo the sampled side;
  * a material's eta is n_interior / n_exterior, the exterior is the side of +n;
  * f carries the cosine |wo.n|, and the transmission lobe carries the radiance factor
    (n_i / n_o)^2: radiance L / n^2 is invariant along a refracted ray and is carried from wo to wi;
  * seen from below (wi.n < 0) the height field is the same one point-mirrored, so the density of
    visible normals is D_wi'(m) with wi' = -wi and m in the upper hemisphere (D(x, y) = D(-x, -y)).

All directions are arrays of shape (N, 3); all results float64."""
import numpy as np
from math import erf as _erf

GGX, BECKMANN = "ggx", "beckmann"
_verf = np.vectorize(_erf, otypes=[np.float64])


def dot(a, b):
    return (a * b).sum(axis=-1)


def normalize(v):
    return v / np.sqrt(dot(v, v))[..., None]


def upper(h):
    """h or -h, whichever has z >= 0: the microfacet normal a half vector stands for."""
    return h * np.where(h[..., 2] < 0, -1.0, 1.0)[..., None]


# ---------------------------------------------------------------------------------------------
def D(dist, au, av, m):
    """The normal distribution (Heitz 2014 eqs. 87 Beckmann, 85 GGX, anisotropic), 0 below the surface."""
    z = m[..., 2]
    with np.errstate(all="ignore"):
        c2 = z * z
        e = ((m[..., 0] / au) ** 2 + (m[..., 1] / av) ** 2) / c2   # tan^2 (cos^2 phi / au^2 + sin^2 phi / av^2)
        if dist == BECKMANN:
            r = np.exp(-e) / (np.pi * au * av * c2 * c2)
        else:
            r = 1.0 / (np.pi * au * av * c2 * c2 * (1.0 + e) ** 2)
    return np.where(z > 0, r, 0.0)


def projected_alpha(au, av, v):
    """alpha along v's azimuth: sqrt(cos^2 phi au^2 + sin^2 phi av^2) (Heitz 2014 eq. 80)."""
    s2 = v[..., 0] ** 2 + v[..., 1] ** 2
    with np.errstate(all="ignore"):
        a = np.sqrt((v[..., 0] ** 2 * au * au + v[..., 1] ** 2 * av * av) / s2)
    return np.where(s2 > 0, a, au)


def smith(dist, au, av, v, beckmann="fit"):
    """Smith's G1 of direction v without the side check.  GGX: 2 / (1 + sqrt(1 + alpha^2 tan^2)),
    exact.  Beckmann: 'exact' is 2 / (1 + erf(a) + exp(-a^2) / (a sqrt(pi))), a = 1 / (alpha tan);
    'fit' is Walter's eq. 27, which the product uses."""
    z = np.abs(v[..., 2])
    with np.errstate(all="ignore"):
        tan = np.sqrt(np.maximum(0.0, 1.0 - z * z)) / z
        at = projected_alpha(au, av, v) * tan
        if dist == GGX:
            g = 2.0 / (1.0 + np.sqrt(1.0 + at * at))
        else:
            a = 1.0 / at
            if beckmann == "exact":
                g = 2.0 / (1.0 + _verf(a) + np.exp(-a * a) / (a * np.sqrt(np.pi)))
            else:
                g = np.where(a < 1.6, (3.535 * a + 2.181 * a * a) / (1.0 + 2.276 * a + 2.577 * a * a), 1.0)
    return np.where(at > 0, g, 1.0)


def G1(dist, au, av, v, m, beckmann="fit"):
    """Walter eq. 23: 0 unless v sees the front of m from its own side of the macrosurface."""
    with np.errstate(all="ignore"):
        ok = dot(v, m) * v[..., 2] > 0
    return np.where(ok, smith(dist, au, av, v, beckmann), 0.0)


def D_visible(dist, au, av, wi, m, beckmann="fit"):
    """Heitz's density of visible normals, for wi on either side (see the module docstring)."""
    w = wi * np.where(wi[..., 2] < 0, -1.0, 1.0)[..., None]
    return G1(dist, au, av, w, m, beckmann) * np.abs(dot(w, m)) * D(dist, au, av, m) / np.abs(w[..., 2])


# ---------------------------------------------------------------------------------------------
def fresnel_dielectric(cos_i, eta):
    """Unpolarised Fresnel reflectance, cos_i >= 0 on the incident side, eta = n_t / n_i; 1 under
    total internal reflection."""
    with np.errstate(all="ignore"):
        st2 = (1.0 - cos_i * cos_i) / (eta * eta)
        ct = np.sqrt(np.maximum(0.0, 1.0 - st2))
        rs = (cos_i - eta * ct) / (cos_i + eta * ct)
        rp = (eta * cos_i - ct) / (eta * cos_i + ct)
    return np.where(st2 >= 1.0, 1.0, 0.5 * (rs * rs + rp * rp))


def fresnel_conductor(cos_i, eta, k):
    """Unpolarised Fresnel reflectance of a conductor of index n + ik seen from index 1, through
    complex arithmetic: the mean of |r_s|^2 and |r_p|^2 with cos_t = sqrt(1 - sin^2 / n^2)."""
    n = np.asarray(eta, np.float64) + 1j * np.asarray(k, np.float64)
    ci = np.asarray(cos_i, np.float64)[..., None].astype(np.complex128)
    ct = np.sqrt(1.0 - (1.0 - ci * ci) / (n * n))
    rs = (ci - n * ct) / (ci + n * ct)
    rp = (n * ci - ct) / (n * ci + ct)
    return 0.5 * (np.abs(rs) ** 2 + np.abs(rp) ** 2)


# ---------------------------------------------------------------------------------------------
def half_reflect(wi, wo):
    return upper(normalize(wi + wo))


def half_refract(wi, wo, n_i, n_o):
    """Walter eq. 16, as the microfacet normal (upper hemisphere)."""
    return upper(normalize(-(n_i[..., None] * wi + n_o[..., None] * wo)))


def jacobian_reflect(wo, h):
    with np.errstate(all="ignore"):
        return 1.0 / (4.0 * np.abs(dot(wo, h)))


def jacobian_refract(wi, wo, h, n_i, n_o):
    with np.errstate(all="ignore"):
        return n_o * n_o * np.abs(dot(wo, h)) / (n_i * dot(wi, h) + n_o * dot(wo, h)) ** 2


class Material:
    """kind 'dielectric' (eta = n_int / n_ext, R, T) or 'conductor' (eta and k per channel, R)."""

    def __init__(self, kind, dist, au, av=None, eta=None, R=(1, 1, 1), T=(1, 1, 1), k=None, two_sided=False):
        self.kind, self.dist, self.au, self.av = kind, dist, float(au), float(au if av is None else av)
        self.eta, self.k = eta, k
        self.R, self.T = np.asarray(R, np.float64), np.asarray(T, np.float64)
        self.two_sided = two_sided


REFLECTION, TRANSMISSION = 1, 2


def _sides(mat, wi):
    """n_i (the index on wi's side) and n_o (the other side's) of a dielectric."""
    up = wi[..., 2] > 0
    return np.where(up, 1.0, mat.eta), np.where(up, mat.eta, 1.0)


def geometry(mat, wi, wo, dh=None):
    """Per pair: is_reflection, the microfacet normal h (nudged by dh and renormalised when dh is
    given, for the conditioning estimate), n_i, n_o."""
    refl = wi[..., 2] * wo[..., 2] > 0
    if mat.kind == "conductor":
        n_i = n_o = np.ones(wi.shape[:-1])
        h = half_reflect(wi, wo)
    else:
        n_i, n_o = _sides(mat, wi)
        with np.errstate(all="ignore"):
            h = np.where(refl[..., None], half_reflect(wi, wo), half_refract(wi, wo, n_i, n_o))
    if dh is not None:
        h = normalize(h + dh)
    return refl, h, n_i, n_o


def f(mat, wi, wo, lobes=REFLECTION | TRANSMISSION, dh=None, beckmann="fit"):
    """The BSDF times |wo.n|, three channels, with the radiance factor on the transmission lobe."""
    refl, h, n_i, n_o = geometry(mat, wi, wo, dh)
    a = (mat.dist, mat.au, mat.av)
    with np.errstate(all="ignore"):
        ih, oh = dot(wi, h), dot(wo, h)
        DG = D(*a, h) * G1(*a, wi, h, beckmann) * G1(*a, wo, h, beckmann)
        if mat.kind == "conductor":
            F = fresnel_conductor(np.abs(ih), mat.eta, mat.k)
            v = mat.R * F * (DG / (4.0 * np.abs(wi[..., 2])))[..., None]
            ok = refl & (wi[..., 2] > 0) & bool(lobes & REFLECTION)
            return np.where(ok[..., None], v, 0.0)
        F = fresnel_dielectric(np.abs(ih), n_o / n_i)
        fr = F * DG / (4.0 * np.abs(wi[..., 2]))
        ft = (np.abs(ih * oh) * n_o * n_o * (1.0 - F) * DG / (np.abs(wi[..., 2]) * (n_i * ih + n_o * oh) ** 2)
              * (n_i / n_o) ** 2)
    fr = np.where(bool(lobes & REFLECTION), fr, 0.0)
    ft = np.where(bool(lobes & TRANSMISSION), ft, 0.0)
    v = np.where(refl[..., None], mat.R * fr[..., None], mat.T * ft[..., None])
    return np.where(np.isfinite(v), v, 0.0)


def pdf(mat, wi, wo, lobes=REFLECTION | TRANSMISSION, dh=None, beckmann="fit", indicator=False):
    """The density of wo: D_wi(h) times the Jacobian, times F or 1 - F when both lobes are asked for.
    indicator: times [G1(wo, h) > 0], the side check that the sampled weight carries (see the product's
    DESIGN.md, Numerics: pdf() of the transmission lobe leaves it out)."""
    refl, h, n_i, n_o = geometry(mat, wi, wo, dh)
    a = (mat.dist, mat.au, mat.av)
    with np.errstate(all="ignore"):
        p = D_visible(*a, wi, h, beckmann)
        if mat.kind == "conductor":
            p = np.where(refl & (wi[..., 2] > 0) & bool(lobes & REFLECTION), p * jacobian_reflect(wo, h), 0.0)
        else:
            p = p * np.where(refl, jacobian_reflect(wo, h), jacobian_refract(wi, wo, h, n_i, n_o))
            if lobes == REFLECTION | TRANSMISSION:
                F = fresnel_dielectric(np.abs(dot(wi, h)), n_o / n_i)
                p = p * np.where(refl, F, 1.0 - F)
            p = np.where(np.where(refl, bool(lobes & REFLECTION), bool(lobes & TRANSMISSION)), p, 0.0)
        if indicator:
            p = np.where(dot(wo, h) * wo[..., 2] > 0, p, 0.0)
    return np.where(np.isfinite(p), p, 0.0)


# ---------------------------------------------------------------------------------------------
# quadratures over the hemisphere, for the self-checks and the expected bin counts
def sphere_dirs(cos, phi):
    s = np.sqrt(np.maximum(0.0, 1.0 - cos * cos))
    return np.stack([s * np.cos(phi), s * np.sin(phi), cos * np.ones_like(phi)], axis=-1)


def hemisphere_integral(fn, n):
    """Integral of fn(m) over the upper hemisphere: the midpoint rule on n x n cells of (theta, phi).
    The integrands here are smooth in phi and periodic, and smooth in theta apart from one kink (where
    wi.m changes sign), so the rule is second order: the error is a third of what halving n moves."""
    th = (np.arange(n) + 0.5) * (0.5 * np.pi / n)
    ph = (np.arange(n) + 0.5) * (2.0 * np.pi / n)
    T, P = np.meshgrid(th, ph, indexing="ij")
    m = sphere_dirs(np.cos(T), P)
    return float((fn(m) * np.sin(T)).sum() * (0.5 * np.pi / n) * (2.0 * np.pi / n))


def refraction_jacobian_numeric(wi, wo, n_i, n_o, step):
    """|dw_h / dw_o| of wo -> h_t(wo) by central differences along two tangents of wo: the area of
    the parallelogram the two difference quotients span.  Second order in the step."""
    t1 = normalize(np.cross(wo, np.array([0.31, -0.52, 0.79])))
    t2 = np.cross(wo, t1)
    d = []
    for t in (t1, t2):
        hp = normalize(-(n_i[..., None] * wi + n_o[..., None] * normalize(wo + step * t)))
        hm = normalize(-(n_i[..., None] * wi + n_o[..., None] * normalize(wo - step * t)))
        d.append((hp - hm) / (2.0 * step))
    c = np.cross(d[0], d[1])
    return np.sqrt(dot(c, c))
