"""numpy float32 restatement, operation by operation, of the reference's dielectric,
thindielectric, conductor and plastic BSDFs, FresnelHelper::fresnelConductorExact and the
BSDFALL two-sided wrapper, read off

    SceneTypes/BSDF_Simple.cu:174-371, 617-660, 765-888     sample / f / pdf
    SceneTypes/BSDF.h:141-207                               BSDFALL (the flip of wi, then of wi and wo)
    SceneTypes/Dispersion.h:26-39,125-168                   Dispersion without dispersion
    Math/FresnelHelper.h:27-57,119-142                      fresnelDielectricExt, fresnelConductorExact
    Math/Frame.h:138-156                                    Frame::reflect / refract
    Math/Vector.h:46,97,369-372, Math/MathFunc.h:112-114,399  dot, lenSqr, normalized, safe_sqrt, rcp

Every operation is one numpy float32 operation (+ - * / sqrt), in the order the reference writes
it.  Nothing here calls a transcendental: the cosine-hemisphere warp of plastic's diffuse lobe is a
callable the test provides (the direction the batch entry returns for a diffuse material), and the
roughconductor is checked against the pinned roughdielectric instead (tests/test_bsdf_host.py).

A material is a dict: type, two_sided, R (m_specularReflectance; plastic: m_diffuseReflectance),
T (m_specularTransmittance), eta, and for types 6-8 ext_eta, ext_k, specular, fdr_int, inv_eta2,
ssw (m_specularSamplingWeight), nonlinear.  A result is (value[3], pdf, wo[3], sampled_type) with
the record's wo / sampledType / pdf as the call leaves them (the caller's initial values where the
reference does not write them)."""
import numpy as np

f32 = np.float32
ENULL, EDIFFUSE_REFLECTION, EGLOSSY_REFLECTION, EDELTA_REFLECTION, EDELTA_TRANSMISSION = 0x1, 0x2, 0x8, 0x20, 0x40
EALL = 0x1ff
ESOLID_ANGLE, EDISCRETE = 1, 4
DIELECTRIC, THINDIELECTRIC, CONDUCTOR, ROUGHCONDUCTOR, PLASTIC = 3, 4, 6, 7, 8
DELTA_EPSILON = f32(1e-3)
INV_PI = f32(1.0) / f32(3.14159265358979)
ZERO3 = (f32(0), f32(0), f32(0))
_0, _1, _2, _4, _half = f32(0), f32(1), f32(2), f32(4), f32(0.5)


def vec(v):
    return (f32(v[0]), f32(v[1]), f32(v[2]))


def dot(a, b):
    r = _0
    r = r + a[0] * b[0]
    r = r + a[1] * b[1]
    r = r + a[2] * b[2]
    return r


def normalize(v):
    ln = np.sqrt(dot(v, v))
    rc = _1 / ln if ln != 0 else _0
    return (v[0] * rc, v[1] * rc, v[2] * rc)


def safe_sqrt(x):
    return np.sqrt(x if x > 0 else _0)


def smul(s, x):   # Spectrum * float
    return (s[0] * x, s[1] * x, s[2] * x)


def sdiv(s, x):   # Spectrum / float: by the reciprocal (Spectrum.h:122-128,150-155)
    recip = _1 / x
    return (s[0] * recip, s[1] * recip, s[2] * recip)


def fresnel_dielectric_ext(cos_i_, eta):
    """-> (F, cosThetaT)"""
    if eta == 1:
        return _0, -cos_i_
    scale = _1 / eta if cos_i_ > 0 else eta
    cos_t_sqr = _1 - (_1 - cos_i_ * cos_i_) * (scale * scale)
    if cos_t_sqr <= 0:
        return _1, _0
    cos_i = abs(cos_i_)
    cos_t = safe_sqrt(cos_t_sqr)
    rs = (cos_i - eta * cos_t) / (cos_i + eta * cos_t)
    rp = (eta * cos_i - cos_t) / (eta * cos_i + cos_t)
    return _half * (rs * rs + rp * rp), (-cos_t if cos_i_ > 0 else cos_t)


def fresnel_conductor_exact(cos_i, eta3, k3):
    out = []
    cos2 = cos_i * cos_i
    sin2 = _1 - cos2
    sin4 = sin2 * sin2
    for eta, k in zip(eta3, k3):
        eta, k = f32(eta), f32(k)
        temp1 = eta * eta - k * k - sin2
        a2pb2 = safe_sqrt(temp1 * temp1 + k * k * eta * eta * _4)
        a = safe_sqrt((a2pb2 + temp1) * _half)
        term1 = a2pb2 + cos2
        term2 = a * (_2 * cos_i)
        rs2 = (term1 - term2) / (term1 + term2)
        term3 = a2pb2 * cos2 + sin4
        term4 = term2 * sin2
        rp2 = rs2 * (term3 - term4) / (term3 + term4)
        out.append(_half * (rp2 + rs2))
    return tuple(out)


def reflect(wi):
    return (-wi[0], -wi[1], wi[2])


def refract(wi, cos_t, eta, inv_eta):
    scale = -(inv_eta if cos_t < 0 else eta)
    return normalize((scale * wi[0], scale * wi[1], cos_t))


def _eta_of(m):   # DispersionCauchy::calc_eta(600) with C = 0
    eta = f32(m["eta"]) + _0 / (f32(600) / f32(1e3))
    return eta, _1 / eta


def _off_delta(a, b):   # math::abs(dot(a, b) - 1) > DeltaEpsilon
    return abs(dot(a, b) - _1) > DELTA_EPSILON


# ---------------------------------------------------------------------------------------------
def dielectric_sample(m, wi, mask, sample, st):
    refl_, trans = (mask & EDELTA_REFLECTION) != 0, (mask & EDELTA_TRANSMISSION) != 0
    eta, inv_eta = _eta_of(m)
    F, cos_t = fresnel_dielectric_ext(wi[2], eta)
    R, T = vec(m["R"]), vec(m["T"])
    f_o = (_1, _1, _1)
    fT = (f_o[0] * T[0], f_o[1] * T[1], f_o[2] * T[2])
    if refl_ and trans:
        if f32(sample[0]) <= F:
            return R, F, reflect(wi), EDELTA_REFLECTION
        factor = inv_eta if cos_t < 0 else eta
        return smul(fT, factor * factor), (_1 - F) * _1, refract(wi, cos_t, eta, inv_eta), EDELTA_TRANSMISSION
    if refl_:
        return R, _1, reflect(wi), EDELTA_REFLECTION
    if trans:
        factor = inv_eta if cos_t < 0 else eta
        return smul(fT, factor * factor * (_1 - F)), _1 * _1, refract(wi, cos_t, eta, inv_eta), EDELTA_TRANSMISSION
    return ZERO3, st[0], st[1], st[2]


def dielectric_f(m, wi, wo, mask, measure):
    refl_ = bool(mask & EDELTA_REFLECTION) and measure == EDISCRETE
    trans = bool(mask & EDELTA_TRANSMISSION) and measure == EDISCRETE
    eta, inv_eta = _eta_of(m)
    F, cos_t = fresnel_dielectric_ext(wi[2], eta)
    if wi[2] * wo[2] >= 0:
        if not refl_ or _off_delta(reflect(wi), wo):
            return ZERO3
        return smul(vec(m["R"]), F)
    if not trans or _off_delta(refract(wi, cos_t, eta, inv_eta), wo):
        return ZERO3
    factor = inv_eta if cos_t < 0 else eta
    T = vec(m["T"])
    return smul(smul(smul((_1 * T[0], _1 * T[1], _1 * T[2]), factor), factor), _1 - F)


def dielectric_pdf(m, wi, wo, mask, measure):
    refl_ = bool(mask & EDELTA_REFLECTION) and measure == EDISCRETE
    trans = bool(mask & EDELTA_TRANSMISSION) and measure == EDISCRETE
    eta, inv_eta = _eta_of(m)
    F, cos_t = fresnel_dielectric_ext(wi[2], eta)
    if wi[2] * wo[2] >= 0:
        if not refl_ or _off_delta(reflect(wi), wo):
            return _0
        return _1 * F if trans else _1
    if not trans or _off_delta(refract(wi, cos_t, eta, inv_eta), wo):
        return _0
    return _1 - F if refl_ else _1 * _1


# ---------------------------------------------------------------------------------------------
def thin_R(m, wi):
    R, _ = fresnel_dielectric_ext(abs(wi[2]), f32(m["eta"]))
    T = _1 - R
    if R < 1:
        R = R + T * T * R / (_1 - R * R)
    return R


def _neg(v):
    return (-v[0], -v[1], -v[2])


def thin_sample(m, wi, mask, sample, st):
    refl_, trans = (mask & EDELTA_REFLECTION) != 0, (mask & ENULL) != 0
    R = thin_R(m, wi)
    Rs, Ts = vec(m["R"]), vec(m["T"])
    if refl_ and trans:
        if f32(sample[0]) <= R:
            return Rs, R, reflect(wi), EDELTA_REFLECTION
        return Ts, _1 - R, _neg(wi), ENULL
    if refl_:
        return smul(Rs, R), _1, reflect(wi), EDELTA_REFLECTION
    if trans:
        return smul(Ts, _1 - R), _1, _neg(wi), ENULL
    return ZERO3, st[0], st[1], st[2]


def thin_f(m, wi, wo, mask, measure):
    refl_ = bool(mask & EDELTA_REFLECTION) and measure == EDISCRETE
    trans = bool(mask & ENULL) and measure == EDISCRETE
    R = thin_R(m, wi)
    if wi[2] * wo[2] >= 0:
        if not refl_ or _off_delta(reflect(wi), wo):
            return ZERO3
        return smul(vec(m["R"]), R)
    if not trans or _off_delta(_neg(wi), wo):
        return ZERO3
    return smul(vec(m["T"]), _1 - R)


def thin_pdf(m, wi, wo, mask, measure):
    refl_ = bool(mask & EDELTA_REFLECTION) and measure == EDISCRETE
    trans = bool(mask & ENULL) and measure == EDISCRETE
    R = thin_R(m, wi)
    if wi[2] * wo[2] >= 0:
        if not refl_ or _off_delta(reflect(wi), wo):
            return _0
        return R if trans else _1
    if not trans or _off_delta(_neg(wi), wo):
        return _0
    return _1 - R if refl_ else _1


# ---------------------------------------------------------------------------------------------
def _spec_mul(a, b):
    return (a[0] * b[0], a[1] * b[1], a[2] * b[2])


def conductor_sample(m, wi, mask, sample, st):
    if not (mask & EDELTA_REFLECTION) or wi[2] <= 0:
        return ZERO3, st[0], st[1], st[2]
    return (_spec_mul(vec(m["R"]), fresnel_conductor_exact(wi[2], m["ext_eta"], m["ext_k"])), _1, reflect(wi),
            EDELTA_REFLECTION)


def _conductor_valid(wi, wo, mask, measure):
    return not (not (mask & EDELTA_REFLECTION) or measure != EDISCRETE or wi[2] <= 0 or wo[2] <= 0 or
                _off_delta(reflect(wi), wo))


def conductor_f(m, wi, wo, mask, measure):
    if not _conductor_valid(wi, wo, mask, measure):
        return ZERO3
    return _spec_mul(vec(m["R"]), fresnel_conductor_exact(wi[2], m["ext_eta"], m["ext_k"]))


def conductor_pdf(m, wi, wo, mask, measure):
    return _1 if _conductor_valid(wi, wo, mask, measure) else _0


# ---------------------------------------------------------------------------------------------
def _plastic_diff(m, Rd):
    fdr = f32(m["fdr_int"])
    if m["nonlinear"]:
        return (Rd[0] / (_1 - Rd[0] * fdr), Rd[1] / (_1 - Rd[1] * fdr), Rd[2] / (_1 - Rd[2] * fdr))
    return sdiv(Rd, _1 - fdr)


def plastic_prob_specular(m, Fi):
    w = f32(m["ssw"])
    return (Fi * w) / (Fi * w + (_1 - Fi) * (_1 - w))


def plastic_remap(m, wi, mask, sample):
    """The sample the diffuse lobe hands to squareToCosineHemisphere, or None when another branch runs."""
    spec_, diff = (mask & EDELTA_REFLECTION) != 0, (mask & EDIFFUSE_REFLECTION) != 0
    if (not diff and not spec_) or wi[2] <= 0 or not diff:
        return None
    if not spec_:
        return (f32(sample[0]), f32(sample[1]))
    Fi, _ = fresnel_dielectric_ext(wi[2], f32(m["eta"]))
    p = plastic_prob_specular(m, Fi)
    if f32(sample[0]) < p:
        return None
    return ((f32(sample[0]) - p) / (_1 - p), f32(sample[1]))


def plastic_sample(m, wi, mask, sample, st, warp):
    """warp(sample2) -> Warp::squareToCosineHemisphere(sample2), from a pinned path."""
    spec_, diff = (mask & EDELTA_REFLECTION) != 0, (mask & EDIFFUSE_REFLECTION) != 0
    if (not diff and not spec_) or wi[2] <= 0:
        return ZERO3, st[0], st[1], st[2]
    eta = f32(m["eta"])
    Fi, _ = fresnel_dielectric_ext(wi[2], eta)
    Rs, Rd, inv_eta2 = vec(m["specular"]), vec(m["R"]), f32(m["inv_eta2"])
    if diff and spec_:
        p = plastic_prob_specular(m, Fi)
        if f32(sample[0]) < p:
            return sdiv(smul(Rs, Fi), p), p, reflect(wi), EDELTA_REFLECTION
        wo = warp(((f32(sample[0]) - p) / (_1 - p), f32(sample[1])))
        Fo, _ = fresnel_dielectric_ext(wo[2], eta)
        d = _plastic_diff(m, Rd)
        return smul(d, inv_eta2 * (_1 - Fi) * (_1 - Fo) / (_1 - p)), (_1 - p) * (INV_PI * wo[2]), wo, EDIFFUSE_REFLECTION
    if spec_:
        return smul(Rs, Fi), _1, reflect(wi), EDELTA_REFLECTION
    wo = warp((f32(sample[0]), f32(sample[1])))
    Fo, _ = fresnel_dielectric_ext(wo[2], eta)
    d = _plastic_diff(m, Rd)
    return smul(d, inv_eta2 * (_1 - Fi) * (_1 - Fo)), INV_PI * wo[2], wo, EDIFFUSE_REFLECTION


def plastic_f(m, wi, wo, mask, measure):
    spec_ = bool(mask & EDELTA_REFLECTION) and measure == EDISCRETE
    diff = bool(mask & EDIFFUSE_REFLECTION) and measure == ESOLID_ANGLE
    if wo[2] <= 0 or wi[2] <= 0:
        return ZERO3
    eta = f32(m["eta"])
    Fi, _ = fresnel_dielectric_ext(wi[2], eta)
    if spec_:
        if abs(dot(reflect(wi), wo) - _1) < DELTA_EPSILON:
            return smul(vec(m["specular"]), Fi)
    elif diff:
        Fo, _ = fresnel_dielectric_ext(wo[2], eta)
        d = _plastic_diff(m, vec(m["R"]))
        return smul(d, (INV_PI * wo[2]) * f32(m["inv_eta2"]) * (_1 - Fi) * (_1 - Fo))
    return ZERO3


def plastic_pdf(m, wi, wo, mask, measure):
    spec_, diff = (mask & EDELTA_REFLECTION) != 0, (mask & EDIFFUSE_REFLECTION) != 0
    if wo[2] <= 0 or wi[2] <= 0:
        return _0
    p = _1 if spec_ else _0
    if spec_ and diff:
        Fi, _ = fresnel_dielectric_ext(wi[2], f32(m["eta"]))
        p = plastic_prob_specular(m, Fi)
    if spec_ and measure == EDISCRETE:
        if abs(dot(reflect(wi), wo) - _1) < DELTA_EPSILON:
            return p
    elif diff and measure == ESOLID_ANGLE:
        return (INV_PI * wo[2]) * (_1 - p)
    return _0


# ---------------------------------------------------------------------------------------------
_SAMPLE = {DIELECTRIC: dielectric_sample, THINDIELECTRIC: thin_sample, CONDUCTOR: conductor_sample}
_F = {DIELECTRIC: dielectric_f, THINDIELECTRIC: thin_f, CONDUCTOR: conductor_f, PLASTIC: plastic_f}
_PDF = {DIELECTRIC: dielectric_pdf, THINDIELECTRIC: thin_pdf, CONDUCTOR: conductor_pdf, PLASTIC: plastic_pdf}


def bsdfall(m, op, wi, wo, mask, measure, sample, warp=None):
    """BSDFALL::sample / f / pdf (op 0 / 1 / 2): start_two_sided<true, false>, the call,
    end_two_sided<true, true>.  -> (value[3], pdf, wo[3], sampled_type); the record starts with the
    query's wo, pdf 0 and sampledType 0."""
    wi, wo = vec(wi), vec(wo)
    flip = wi[2] < 0 and m["two_sided"]
    if flip:
        wi = (wi[0], wi[1], wi[2] * f32(-1))
    value, pdf, st = ZERO3, _0, 0
    with np.errstate(all="ignore"):
        if op == 0:
            init = (_0, wo, 0)
            if m["type"] == PLASTIC:
                value, pdf, wo, st = plastic_sample(m, wi, mask, sample, init, warp)
            else:
                value, pdf, wo, st = _SAMPLE[m["type"]](m, wi, mask, sample, init)
        elif op == 1:
            value = _F[m["type"]](m, wi, wo, mask, measure)
        else:
            pdf = _PDF[m["type"]](m, wi, wo, mask, measure)
    if flip:
        wo = (wo[0], wo[1], wo[2] * f32(-1))
    return value, pdf, wo, st
