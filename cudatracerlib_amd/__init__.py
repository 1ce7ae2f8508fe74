"""cudatracerlib_amd — MI355X-native traversal backend for the CudaTracerLib
hot path (BVH traversal + Woop ray/triangle intersection driven by the
PathTracer pass loop).

The product is ``_lib/libctl_trace.so`` (hand-written gfx950 HIP kernels plus
the C-ABI of ``include/ctl_trace.h``).  This module is a thin host-side mirror
of the reference's surface for that path:

  reference                                   here
  ------------------------------------------- ---------------------------------
  DynamicScene (host scene, Engine/DynamicScene.h:40-188)   HostScene
  UpdateKernel / KernelDynamicScene upload                  Tracer.upload_scene
  __internal__IntersectBuffers (TraceHelper.cu:736-746)     Tracer.intersect_buffers
  PathTracer::DoPass (Kernel/Tracer.h:209-248)              PathTracer.do_pass
  DoPass with an IBlockSampler (Tracer.h:233-237,264-289)   PathTracer.do_pass_adaptive
  VarianceBlockSampler (Kernel/BlockSampler)                BlockSampler
  k_getNumRaysTraced (TraceHelper.cu:309-314)               Tracer.rays_traced

Device memory, streams and torch.distributed come from PyTorch; no torch type
crosses the C-ABI (device pointers are passed as integers).  There is no CPU
fallback: every compute call goes through the HIP library and raises if it is
missing or fails.
"""
import ctypes as C
import os

import numpy as np

from . import _abi
from ._abi import (ImageFilter, Tonemap, LuminanceInfo, CTL_FILTER_BOX, CTL_FILTER_GAUSSIAN, CTL_FILTER_MITCHELL,
                   CTL_FILTER_LANCZOS, CTL_FILTER_TRIANGLE, CTL_FILTER_NLM, CTL_NLM_DIRECT)
from ._abi import MaterialExt, BsdfQuery, BsdfResult
from ._abi import (PTParams, WptParams, PrimParams, SceneDesc, Material, Pixel, Ray, Hit, CTL_SCENE_HALF_HOST_QUIRK, CTL_SCENE_BINARY_BVH,
                   CTL_BSDF_DIFFUSE, CTL_EDIFFUSE_REFLECTION, CTL_PT_MEGAKERNEL, CTL_PT_WAVEFRONT, CTL_PT_RENDER_AHEAD,
                   CTL_COMM_ID_BYTES)

__all__ = ["HostScene", "Tracer", "PathTracer", "BlockSampler", "BLOCK_INFO_DTYPE", "WavefrontPathTracer", "PrimTracer", "PrimParams", "WptParams", "PTParams", "SceneDesc", "Material", "Pixel", "Ray", "Hit",
           "roughdielectric_material", "set_alpha_map", "comm_unique_id", "comm_init_rank", "comm_init_all",
           "comm_destroy", "ImageFilter", "Tonemap", "LuminanceInfo", "image_filter", "filter_evaluate", "rgbe_encode",
           "rgbe_decode", "tonemap_constants", "CTL_FILTER_BOX", "CTL_FILTER_GAUSSIAN", "CTL_FILTER_MITCHELL",
           "CTL_FILTER_LANCZOS", "CTL_FILTER_TRIANGLE", "CTL_FILTER_NLM", "CTL_NLM_DIRECT",
           "CTL_SCENE_HALF_HOST_QUIRK", "CTL_SCENE_BINARY_BVH", "CTL_PT_MEGAKERNEL", "CTL_PT_WAVEFRONT", "CTL_PT_RENDER_AHEAD", "lib", "diffuse_material",
           "MaterialExt", "BsdfQuery", "BsdfResult", "BSDF_QUERY_DTYPE", "BSDF_RESULT_DTYPE", "dielectric_material",
           "thindielectric_material", "conductor_material", "roughconductor_material", "plastic_material",
           "fresnel_diffuse_reflectance", "host_bsdf_eval", "host_math_eval", "MATH_FUNCTIONS",
           "LIGHT_QUERY_DTYPE", "LIGHT_RESULT_DTYPE", "host_light_eval",
           "MEDIUM_QUERY_DTYPE", "MEDIUM_RESULT_DTYPE", "host_medium_eval",
           "SENSOR_QUERY_DTYPE", "SENSOR_RESULT_DTYPE", "SENSOR_KINDS", "host_sensor_eval"]


def lib():
    return _abi.load()


class CTLError(RuntimeError):
    pass


def _check(status, ctx=None, what=""):
    if status != 0:
        L = lib()
        msg = L.ctl_last_error(ctx) if ctx is not None else L.ctl_host_last_error()
        raise CTLError(f"{what} failed (status {status}): {msg.decode() if msg else ''}")


def set_alpha_map(m, state, threshold, alpha_texture=None):
    """Material::AlphaMap (Engine/Material.h:14-36): state 1/2 = luminance/alpha of
    `alpha_texture`, 5/6 = luminance/alpha of the diffuse reflectance texture."""
    m.alpha_state = int(state)
    m.alpha_texture = 0xFFFFFFFF if alpha_texture is None else int(alpha_texture)
    m.alpha_threshold = float(threshold)
    return m


def diffuse_material(r, g, b, two_sided=True, texture=None):
    """diffuse BSDF (BSDF_Simple.cu:7-75); `texture` = ImageTexture index of
    m_reflectance (HostScene.add_texture), else the constant (r, g, b)."""
    m = Material()
    m.alpha_texture = 0xFFFFFFFF
    m.bsdf_type = CTL_BSDF_DIFFUSE
    m.combined_type = CTL_EDIFFUSE_REFLECTION
    m.two_sided = 1 if two_sided else 0
    m.node_light_index = 0xFFFFFFFF
    m.reflectance[:] = [r, g, b]
    m.texture = 0xFFFFFFFF if texture is None else int(texture)
    return m


def roughdielectric_material(distribution, eta, alpha_u, alpha_v=None, reflectance=(1.0, 1.0, 1.0),
                             transmittance=(1.0, 1.0, 1.0)):
    """roughdielectric BSDF (BSDF_Simple.cu:373-615) with constant textures;
    distribution = _abi.CTL_MICROFACET_BECKMANN or _abi.CTL_MICROFACET_GGX."""
    m = Material()
    m.alpha_texture = 0xFFFFFFFF
    m.bsdf_type = _abi.CTL_BSDF_ROUGHDIELECTRIC
    m.combined_type = _abi.CTL_EGLOSSY_REFLECTION | _abi.CTL_EGLOSSY_TRANSMISSION
    m.two_sided = 0
    m.node_light_index = 0xFFFFFFFF
    m.reflectance[:] = list(reflectance)
    m.texture = 0xFFFFFFFF
    m.transmittance[:] = list(transmittance)
    m.distribution = int(distribution)
    m.eta = float(eta)
    m.inv_eta = float(np.float32(1.0) / np.float32(eta))      # roughdielectric::Update
    m.alpha_u = float(alpha_u)
    m.alpha_v = float(alpha_u if alpha_v is None else alpha_v)
    m.sample_visible = 1                                         # getSampleVisible(Beckmann/GGX, true)
    return m


def _specular_material(bsdf_type, combined, eta, reflectance, transmittance, two_sided):
    m = Material()
    m.alpha_texture = 0xFFFFFFFF
    m.bsdf_type = int(bsdf_type)
    m.combined_type = int(combined)
    m.two_sided = 1 if two_sided else 0
    m.node_light_index = 0xFFFFFFFF
    m.reflectance[:] = list(reflectance)
    m.texture = 0xFFFFFFFF
    m.transmittance[:] = list(transmittance)
    m.eta = float(eta)
    m.inv_eta = float(np.float32(1.0) / np.float32(eta)) if eta else 0.0
    return m


def dielectric_material(eta=1.5, reflectance=(1.0, 1.0, 1.0), transmittance=(1.0, 1.0, 1.0), two_sided=False):
    """dielectric BSDF (BSDF_Simple.cu:174-277) without dispersion: eta = DispersionCauchy B, C = 0."""
    return _specular_material(_abi.CTL_BSDF_DIELECTRIC, _abi.CTL_EDELTA_REFLECTION | _abi.CTL_EDELTA_TRANSMISSION, eta,
                              reflectance, transmittance, two_sided)


def thindielectric_material(eta=1.5, reflectance=(1.0, 1.0, 1.0), transmittance=(1.0, 1.0, 1.0), two_sided=False):
    """thindielectric BSDF (BSDF_Simple.cu:279-371)."""
    return _specular_material(_abi.CTL_BSDF_THINDIELECTRIC, _abi.CTL_EDELTA_REFLECTION | _abi.CTL_EDELTA_TRANSMISSION,
                              eta, reflectance, transmittance, two_sided)


def conductor_material(eta, k, reflectance=(1.0, 1.0, 1.0), two_sided=False):
    """conductor BSDF (BSDF_Simple.cu:617-660): (Material, MaterialExt); eta, k are rgb triples."""
    m = _specular_material(_abi.CTL_BSDF_CONDUCTOR, _abi.CTL_EDELTA_REFLECTION, 0.0, reflectance, (0.0, 0.0, 0.0),
                           two_sided)
    e = MaterialExt()
    e.eta[:] = list(eta)
    e.k[:] = list(k)
    return m, e


def roughconductor_material(distribution, eta, k, alpha_u, alpha_v=None, reflectance=(1.0, 1.0, 1.0), two_sided=False):
    """roughconductor BSDF (BSDF_Simple.cu:662-763) with constant textures: (Material, MaterialExt)."""
    m, e = conductor_material(eta, k, reflectance, two_sided)
    m.bsdf_type = _abi.CTL_BSDF_ROUGHCONDUCTOR
    m.combined_type = _abi.CTL_EGLOSSY_REFLECTION
    m.distribution = int(distribution)
    m.alpha_u = float(alpha_u)
    m.alpha_v = float(alpha_u if alpha_v is None else alpha_v)
    m.sample_visible = 1                                         # getSampleVisible(Beckmann/GGX, true)
    return m, e


def _fresnel_dielectric_ext(cos_i, eta):
    """FresnelHelper::fresnelDielectricExt(cosThetaI, eta) in float32 (FresnelHelper.h:27-57,191-195)."""
    f = np.float32
    cos_i, eta = f(cos_i), f(eta)
    if eta == 1:
        return f(0)
    scale = f(1) / eta if cos_i > 0 else eta
    t2 = f(1) - (f(1) - cos_i * cos_i) * (scale * scale)
    if t2 <= 0:
        return f(1)
    ci, ct = abs(cos_i), np.sqrt(max(f(0), t2))
    rs = (ci - eta * ct) / (ci + eta * ct)
    rp = (eta * ci - ct) / (eta * ci + ct)
    return f(0.5) * (rs * rs + rp * rp)


def fresnel_diffuse_reflectance(eta):
    """FresnelHelper::fresnelDiffuseReflectance(eta, false) (FresnelHelper.cu:13-62): the adaptive
    Gauss-Lobatto quadrature GaussLobattoIntegrator(1024, 0, 1e-5) of Math/Integrator.h:28-153 over
    fresnelDielectricExt(sqrt(xi), eta), xi in [0, 1], restated in float32 (sub-intervals left to right)."""
    f = np.float32
    eta = f(eta)
    fn = lambda xi: _fresnel_dielectric_ext(np.sqrt(f(xi)), eta)   # noqa: E731
    alpha, beta = np.sqrt(f(2.0) / f(3.0)), f(1.0) / np.sqrt(f(5.0))
    x1, x2, x3 = f(0.94288241569547971906), f(0.64185334234578130578), f(0.23638319966214988028)
    a, b = f(0), f(1)
    max_evals, rel_error, eps, flt_max = 1024, f(1e-5), np.finfo(f).eps, np.finfo(f).max
    m, h = (a + b) / f(2), (b - a) / f(2)
    y1, y3, y5, y7, y9, y11, y13 = (fn(a), fn(m - alpha * h), fn(m - beta * h), fn(m), fn(m + beta * h),
                                    fn(m + alpha * h), fn(b))
    acc = h * (f(0.0158271919734801831) * (y1 + y13) + f(0.0942738402188500455) * (fn(m - x1 * h) + fn(m + x1 * h)) +
               f(0.1550719873365853963) * (y3 + y11) + f(0.1888215739601824544) * (fn(m - x2 * h) + fn(m + x2 * h)) +
               f(0.1997734052268585268) * (y5 + y9) + f(0.2249264653333395270) * (fn(m - x3 * h) + fn(m + x3 * h)) +
               f(0.2426110719014077338) * y7)
    evals = [13]
    i2 = (h / f(6)) * (y1 + y13 + f(5) * (y5 + y9))
    i1 = (h / f(1470)) * (f(77) * (y1 + y13) + f(432) * (y3 + y11) + f(625) * (y5 + y9) + f(672) * y7)
    r = f(1)
    if abs(i2 - acc) != 0:
        r = abs(i1 - acc) / abs(i2 - acc)
    if r == 0 or r > 1:
        r = f(1)
    tol = flt_max
    if acc != 0:
        tol = acc * max(rel_error, eps) / (r * eps)
    evals[0] += 2

    def step(a, b, fa, fb):
        h, m = (b - a) / f(2), (a + b) / f(2)
        mll, ml, mr, mrr = m - alpha * h, m - beta * h, m + beta * h, m + alpha * h
        fmll, fml, fm, fmr, fmrr = fn(mll), fn(ml), fn(m), fn(mr), fn(mrr)
        i2 = (h / f(6)) * (fa + fb + f(5) * (fml + fmr))
        i1 = (h / f(1470)) * (f(77) * (fa + fb) + f(432) * (fmll + fmrr) + f(625) * (fml + fmr) + f(672) * fm)
        evals[0] += 5
        if evals[0] >= max_evals:
            return i1
        dist = tol + (i1 - i2)
        if dist == tol or mll <= a or b <= mrr:
            return i1
        return (step(a, mll, fa, fmll) + step(mll, ml, fmll, fml) + step(ml, m, fml, fm) + step(m, mr, fm, fmr) +
                step(mr, mrr, fmr, fmrr) + step(mrr, b, fmrr, fb))

    with np.errstate(over="ignore"):
        return f(f(1) * step(a, b, fn(a), fn(b)))


def plastic_material(eta=1.5, diffuse=(0.5, 0.5, 0.5), specular=(1.0, 1.0, 1.0), nonlinear=False, texture=None,
                     diffuse_average=None, two_sided=False):
    """plastic BSDF (BSDF_Simple.cu:765-888): (Material, MaterialExt) with the members plastic::Update()
    derives (BSDF_Simple.h:259-266).  `texture` = ImageTexture index of m_diffuseReflectance; pass its
    average colour as `diffuse_average` (Texture::Average) for the specular sampling weight, which
    otherwise uses `diffuse`."""
    f = np.float32
    m = _specular_material(_abi.CTL_BSDF_PLASTIC, _abi.CTL_EDELTA_REFLECTION | _abi.CTL_EDIFFUSE_REFLECTION, eta, diffuse,
                           (0.0, 0.0, 0.0), two_sided)
    m.texture = 0xFFFFFFFF if texture is None else int(texture)
    e = MaterialExt()
    e.specular[:] = list(specular)
    e.inv_eta2 = float(f(1) / (f(eta) * f(eta)))
    e.fdr_int = float(fresnel_diffuse_reflectance(f(1) / f(eta)))
    lum = lambda c: f(c[0]) * f(0.212671) + f(c[1]) * f(0.715160) + f(c[2]) * f(0.072169)   # noqa: E731  Spectrum::getLuminance
    d_avg, s_avg = lum(diffuse if diffuse_average is None else diffuse_average), lum(specular)
    e.specular_sampling_weight = float(s_avg / (d_avg + s_avg))
    e.nonlinear = 1 if nonlinear else 0
    return m, e


BSDF_QUERY_DTYPE = np.dtype([("material", "<u4"), ("op", "<u4"), ("type_mask", "<u4"), ("measure", "<u4"),
                             ("wi", "<f4", 3), ("wo", "<f4", 3), ("sample", "<f4", 2), ("uv", "<f4", 2)])
BSDF_RESULT_DTYPE = np.dtype([("value", "<f4", 3), ("pdf", "<f4"), ("wo", "<f4", 3), ("sampled_type", "<u4")])


def host_bsdf_eval(desc, queries):
    """BSDFALL::sample / f / pdf of desc's materials for an array of BSDF_QUERY_DTYPE queries, on the
    CPU (ctl_host_bsdf_eval): BSDF_RESULT_DTYPE results, the device entry's arithmetic bit for bit."""
    q = np.ascontiguousarray(queries, dtype=BSDF_QUERY_DTYPE)
    out = np.zeros(q.shape[0], dtype=BSDF_RESULT_DTYPE)
    _check(lib().ctl_host_bsdf_eval(C.byref(desc), q.shape[0], q.ctypes.data, out.ctypes.data), None,
           "ctl_host_bsdf_eval")
    return out


LIGHT_QUERY_DTYPE = np.dtype([("light", "<u4"), ("ref", "<f4", 3), ("ref_n", "<f4", 3), ("sample", "<f4", 2)])
LIGHT_RESULT_DTYPE = np.dtype([("value", "<f4", 3), ("pdf", "<f4"), ("d", "<f4", 3), ("dist", "<f4"), ("p", "<f4", 3),
                               ("measure", "<u4"), ("n", "<f4", 3), ("pad", "<u4")])


def host_light_eval(desc, queries):
    """Light::sampleDirect of desc's lights for an array of LIGHT_QUERY_DTYPE queries, on the CPU
    (ctl_host_light_eval): LIGHT_RESULT_DTYPE results, the device entry's arithmetic bit for bit."""
    q = np.ascontiguousarray(queries, dtype=LIGHT_QUERY_DTYPE)
    out = np.zeros(q.shape[0], dtype=LIGHT_RESULT_DTYPE)
    _check(lib().ctl_host_light_eval(C.byref(desc), q.ctypes.data, q.shape[0], out.ctypes.data), None,
           "ctl_host_light_eval")
    return out


MEDIUM_QUERY_DTYPE = np.dtype([("op", "<u4"), ("ori", "<f4", 3), ("dir", "<f4", 3), ("wo", "<f4", 3), ("tmin", "<f4"),
                               ("tmax", "<f4"), ("u", "<f4", 2)])
MEDIUM_RESULT_DTYPE = np.dtype([("hit", "<u4"), ("t0", "<f4"), ("t1", "<f4"), ("t", "<f4"), ("p", "<f4", 3),
                                ("transmittance", "<f4", 3), ("sigma_a", "<f4", 3), ("sigma_s", "<f4", 3),
                                ("pdf_success", "<f4"), ("pdf_success_rev", "<f4"), ("pdf_failure", "<f4"),
                                ("value", "<f4"), ("pdf", "<f4"), ("wo_out", "<f4", 3)])


def host_medium_eval(desc, queries):
    """The medium's five operations (_abi.CTL_MEDIUM_*) of desc's volume for an array of
    MEDIUM_QUERY_DTYPE queries, on the CPU (ctl_host_medium_eval): MEDIUM_RESULT_DTYPE results, the
    device entry's arithmetic bit for bit."""
    q = np.ascontiguousarray(queries, dtype=MEDIUM_QUERY_DTYPE)
    out = np.zeros(q.shape[0], dtype=MEDIUM_RESULT_DTYPE)
    _check(lib().ctl_host_medium_eval(C.byref(desc), q.ctypes.data, q.shape[0], out.ctypes.data), None,
           "ctl_host_medium_eval")
    return out


SENSOR_QUERY_DTYPE = np.dtype([("pixel_sample", "<f4", 2), ("aperture_sample", "<f4", 2), ("differential", "<u4")])
SENSOR_RESULT_DTYPE = np.dtype([("o", "<f4", 3), ("d", "<f4", 3), ("ox", "<f4", 3), ("dx", "<f4", 3), ("oy", "<f4", 3),
                                ("dy", "<f4", 3), ("has_differentials", "<u4"), ("pad", "<u4")])
# HostScene.set_sensor kinds -> the reference's sensor type ids (_abi.CTL_SENSOR_*)
SENSOR_KINDS = {"spherical": _abi.CTL_SENSOR_SPHERICAL, "perspective": _abi.CTL_SENSOR_PERSPECTIVE,
                "thinlens": _abi.CTL_SENSOR_THINLENS, "orthographic": _abi.CTL_SENSOR_ORTHOGRAPHIC,
                "telecentric": _abi.CTL_SENSOR_TELECENTRIC}


def host_sensor_eval(desc, queries):
    """Sensor::sampleRay (differential = 0) or Sensor::sampleRayDifferential of desc's sensor for an array of
    SENSOR_QUERY_DTYPE queries, on the CPU (ctl_host_sensor_eval): SENSOR_RESULT_DTYPE results, the device
    entry's arithmetic bit for bit."""
    q = np.ascontiguousarray(queries, dtype=SENSOR_QUERY_DTYPE)
    out = np.zeros(q.shape[0], dtype=SENSOR_RESULT_DTYPE)
    _check(lib().ctl_host_sensor_eval(C.byref(desc), q.ctypes.data, q.shape[0], out.ctypes.data), None,
           "ctl_host_sensor_eval")
    return out


MATH_FUNCTIONS = {name: i for i, name in enumerate(_abi.CTL_MATH_FUNCTIONS)}   # name -> CTL_MATH_* id


def _math_fn(fn):
    return MATH_FUNCTIONS[fn] if isinstance(fn, str) else int(fn)


def host_math_eval(fn, a, b=None):
    """The scalar arithmetic of the kernels on the CPU (ctl_host_math_eval): function `fn` (a name of
    MATH_FUNCTIONS or its id) of the 32-bit words of `a` (float32, or uint32 bit patterns) and, for atan2,
    pow and div, of `b`; returns uint32 result words, the device entry's arithmetic bit for bit.
    normal_encode16 takes n x 3 floats, normal_decode16 returns n x 3 words."""
    fn = _math_fn(fn)
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 4, a.dtype
    n = a.size // 3 if fn == MATH_FUNCTIONS["normal_encode16"] else a.size
    if b is not None:
        b = np.ascontiguousarray(b)
        assert b.dtype.itemsize == 4 and b.size == n, (b.dtype, b.size)
    out = np.zeros((n, 3) if fn == MATH_FUNCTIONS["normal_decode16"] else n, dtype=np.uint32)
    _check(lib().ctl_host_math_eval(fn, n, a.ctypes.data, b.ctypes.data if b is not None else None, out.ctypes.data),
           None, "ctl_host_math_eval")
    return out


# the reference's default parameters per filter type: (x_width, y_width, a, b)
_FILTER_DEFAULTS = {CTL_FILTER_BOX: (1.0, 1.0, 0.0, 0.0), CTL_FILTER_GAUSSIAN: (2.0, 2.0, -2.0, 0.0),
                    CTL_FILTER_MITCHELL: (2.0, 2.0, 1.0 / 3.0, 1.0 / 3.0), CTL_FILTER_LANCZOS: (6.0, 6.0, 3.0, 0.0),
                    CTL_FILTER_TRIANGLE: (2.0, 2.0, 0.0, 0.0), CTL_FILTER_NLM: (0.0, 0.0, 0.0, 0.0)}


def image_filter(type, x_width=None, y_width=None, a=None, b=None, k=0.45, sigma2_scale=0.005, update_periodicity=25,
                 flags=0):
    """An ImageFilter (ctl_image_filter) of `type` with the reference's defaults (SceneTypes/Filter.h
    constructors, NonLocalMeansFilter's settings) for every parameter left None."""
    d = _FILTER_DEFAULTS.get(int(type), (0.0, 0.0, 0.0, 0.0))
    v = [d[i] if x is None else float(x) for i, x in enumerate((x_width, y_width, a, b))]
    return ImageFilter(int(type), v[0], v[1], v[2], v[3], float(k), float(sigma2_scale), int(update_periodicity),
                       int(flags))


def filter_evaluate(filter, x, y):
    """Filter::Evaluate(x, y) of a canonical filter as the kernels compute it (ctl_filter_evaluate, host)."""
    out = C.c_float()
    _check(lib().ctl_filter_evaluate(C.byref(filter), float(x), float(y), C.byref(out)), None, "ctl_filter_evaluate")
    return np.float32(out.value)


def rgbe_encode(rgb):
    """Spectrum::toRGBE of linear (r, g, b): one uint32, r in the low byte (ctl_rgbe_encode, host)."""
    v = (C.c_float * 3)(*np.asarray(rgb, dtype=np.float32).reshape(3).tolist())
    out = C.c_uint32()
    _check(lib().ctl_rgbe_encode(v, C.byref(out)), None, "ctl_rgbe_encode")
    return int(out.value)


def rgbe_decode(word):
    """Spectrum::fromRGBE as float32[3] (ctl_rgbe_decode, host)."""
    v = (C.c_float * 3)()
    _check(lib().ctl_rgbe_decode(int(word) & 0xFFFFFFFF, v), None, "ctl_rgbe_decode")
    return np.array(list(v), dtype=np.float32)


def tonemap_constants(tonemap, avg_log_lum, max_lum):
    """ToneMapPostProcess::Apply's (scale, 1 / Lwhite^2 burn^4) (ctl_tonemap_constants, host)."""
    s, i = C.c_float(), C.c_float()
    _check(lib().ctl_tonemap_constants(C.byref(tonemap), float(avg_log_lum), float(max_lum), C.byref(s), C.byref(i)),
           None, "ctl_tonemap_constants")
    return np.float32(s.value), np.float32(i.value)


class HostScene:
    """Host-side scene compiler (the reference's DynamicScene + Mesh compile)."""

    def __init__(self):
        self._L = lib()
        self._h = self._L.ctl_host_scene_create()
        self.desc = None

    def close(self):
        if self._h:
            self._L.ctl_host_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def generate(self, config, scale=1.0, width=256, height=256):
        _check(self._L.ctl_host_scene_generate(self._h, int(config), float(scale), int(width), int(height)),
               None, "ctl_host_scene_generate")
        return self

    def add_mesh(self, vertices, indices, materials, mat_index=None, normals=None, uvs=None, materials_ext=None):
        """materials: Material records, or (Material, MaterialExt) pairs as conductor_material,
        roughconductor_material and plastic_material return them; materials_ext: the ext records as a
        list of its own (None entries for materials without one)."""
        import numpy as np
        if any(isinstance(m, tuple) for m in materials):
            if materials_ext is not None:
                raise ValueError("add_mesh: give (Material, MaterialExt) pairs or materials_ext, not both")
            materials_ext = [m[1] if isinstance(m, tuple) else None for m in materials]
            materials = [m[0] if isinstance(m, tuple) else m for m in materials]
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        i = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1, 3)
        mats = (Material * len(materials))(*materials)
        mi = None if mat_index is None else np.ascontiguousarray(mat_index, dtype=np.uint8)
        n = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32)
        uv = None if uvs is None else np.ascontiguousarray(uvs, dtype=np.float32)
        self._keep = getattr(self, "_keep", []) + [v, i, mi, n, uv, mats]
        r = self._L.ctl_host_scene_add_mesh(
            self._h, v.ctypes.data, v.shape[0], i.ctypes.data, i.shape[0],
            None if n is None else n.ctypes.data, None if uv is None else uv.ctypes.data,
            None if mi is None else mi.ctypes.data, mats, len(materials))
        if r < 0:
            _check(1, None, "add_mesh")
        if materials_ext is not None and any(e is not None for e in materials_ext):
            if len(materials_ext) != len(materials):
                raise ValueError("add_mesh: one ext record (or None) per material")
            ext = (MaterialExt * len(materials))(*[MaterialExt() if e is None else e for e in materials_ext])
            _check(self._L.ctl_host_scene_set_mesh_material_ext(self._h, r, ext, len(materials)), None,
                   "ctl_host_scene_set_mesh_material_ext")
        return r

    def add_texture(self, rgba, filter=_abi.CTL_TEX_TRILINEAR, wrap=_abi.CTL_WRAP_REPEAT,
                    mapping=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0), scale=(1.0, 1.0, 1.0)):
        """ImageTexture over an (h, w) uint32 RGBA8 image (r in the low byte); returns its index."""
        img = np.ascontiguousarray(rgba, dtype=np.uint32)
        h, w = img.shape
        self._keep = getattr(self, "_keep", []) + [img]
        r = self._L.ctl_host_scene_add_texture(self._h, img.ctypes.data, w, h, int(filter), int(wrap),
                                               (C.c_float * 6)(*mapping), (C.c_float * 3)(*scale))
        if r < 0:
            _check(1, None, "add_texture")
        return r

    def add_animated_mesh(self, vertices, normals, bone_indices, bone_weights, indices, materials, mat_index=None,
                          uvs=None):
        """Skinned mesh (AnimatedMesh): rest pose `vertices`/`normals` (n, 3), 8 bone
        indices and 8 weights (n, 8) uint8 per vertex (weight w means w/255)."""
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        nrm = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        bi = np.ascontiguousarray(bone_indices, dtype=np.uint8).reshape(-1, 8)
        bw = np.ascontiguousarray(bone_weights, dtype=np.uint8).reshape(-1, 8)
        dt = np.dtype([("pos", np.float32, 3), ("normal", np.float32, 3), ("bi", np.uint8, 8), ("bw", np.uint8, 8)])
        assert dt.itemsize == C.sizeof(_abi.AnimVertex)
        rec = np.zeros(v.shape[0], dt)
        rec["pos"], rec["normal"], rec["bi"], rec["bw"] = v, nrm, bi, bw
        av = C.cast(rec.ctypes.data, C.POINTER(_abi.AnimVertex))
        i = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1, 3)
        mats = (Material * len(materials))(*materials)
        mi = None if mat_index is None else np.ascontiguousarray(mat_index, dtype=np.uint8)
        uv = None if uvs is None else np.ascontiguousarray(uvs, dtype=np.float32)
        self._keep = getattr(self, "_keep", []) + [rec, i, mi, uv, mats]
        r = self._L.ctl_host_scene_add_animated_mesh(
            self._h, av, v.shape[0], i.ctypes.data, i.shape[0], None if uv is None else uv.ctypes.data,
            None if mi is None else mi.ctypes.data, mats, len(materials))
        if r < 0:
            _check(1, None, "add_animated_mesh")
        return r

    def add_xmsh(self, data, materials=None, material_record_size=_abi.CTL_XMSH_MATERIAL_RECORD_SIZE):
        """Compiled mesh from an .xmsh stream (bytes or a path) — Mesh::Mesh(path, IInStream&)
        (Engine/Mesh.cpp:46-98).  Reference files: pass sizeof(Material) of the writing build as
        material_record_size and the kernel materials in file order."""
        if isinstance(data, (str, os.PathLike)):
            with open(data, "rb") as f:
                data = f.read()
        buf = C.create_string_buffer(bytes(data), len(data))
        mats = None if materials is None else (Material * len(materials))(*materials)
        r = self._L.ctl_host_scene_add_xmsh(self._h, buf, len(data), int(material_record_size), mats,
                                            0 if materials is None else len(materials))
        if r < 0:
            _check(1, None, "add_xmsh")
        return r

    def write_xmsh(self, mesh, path=None):
        """Mesh `mesh` of the last compile as .xmsh bytes (written to `path` when given)."""
        n = C.c_uint64(0)
        _check(self._L.ctl_host_scene_write_xmsh(self._h, int(mesh), None, 0, C.byref(n)), None, "write_xmsh")
        buf = C.create_string_buffer(n.value)
        _check(self._L.ctl_host_scene_write_xmsh(self._h, int(mesh), buf, n.value, C.byref(n)), None, "write_xmsh")
        data = buf.raw[:n.value]
        if path is not None:
            with open(path, "wb") as f:
                f.write(data)
        return data

    def write_animated_xmsh(self, mesh, path=None):
        """Animated mesh `mesh` of the last compile as an Animated .xmsh stream (type 1:
        the compiled body, then its animations, AnimatedVertex records and triangles)."""
        n = C.c_uint64(0)
        _check(self._L.ctl_host_scene_write_animated_xmsh(self._h, int(mesh), None, 0, C.byref(n)), None,
               "write_animated_xmsh")
        buf = C.create_string_buffer(n.value)
        _check(self._L.ctl_host_scene_write_animated_xmsh(self._h, int(mesh), buf, n.value, C.byref(n)), None,
               "write_animated_xmsh")
        data = buf.raw[:n.value]
        if path is not None:
            with open(path, "wb") as f:
                f.write(data)
        return data

    def set_animated_bvh(self, mode):
        """0 (default): skinned meshes compile with the binned builder, no splits;
        1: with the scene's builder (set_bvh_builder / set_bvh_params)."""
        _check(self._L.ctl_host_scene_set_animated_bvh(self._h, int(mode)), None, "set_animated_bvh")
        return self

    def add_animation(self, mesh, name, frame_rate, frames):
        """Animation of an animated mesh: frames = (n_frames, n_bones, 4, 4) bone matrices.
        Returns its index in the mesh."""
        f = np.ascontiguousarray(frames, dtype=np.float32)
        if f.ndim != 4 or f.shape[2:] != (4, 4):
            raise ValueError("frames must be (n_frames, n_bones, 4, 4)")
        r = self._L.ctl_host_scene_add_animation(self._h, int(mesh), name.encode(), int(frame_rate), f.ctypes.data,
                                                 f.shape[0], f.shape[1])
        if r < 0:
            _check(1, None, "add_animation")
        return r

    def animations(self, mesh):
        """The animations of mesh `mesh` (added or read from an Animated .xmsh): a list of
        dicts {name, frame_rate, frames: (n_frames, n_bones, 4, 4) float32}."""
        n = self._L.ctl_host_scene_animation_count(self._h, int(mesh))
        if n < 0:
            _check(1, None, "animations")
        out = []
        for a in range(n):
            name = C.create_string_buffer(128)
            rate, nf, nb = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
            _check(self._L.ctl_host_scene_animation_info(self._h, int(mesh), a, name, C.byref(rate), C.byref(nf),
                                                         C.byref(nb)), None, "animations")
            m = np.zeros((nf.value, nb.value, 4, 4), np.float32)
            _check(self._L.ctl_host_scene_animation_frames(self._h, int(mesh), a, m.ctypes.data,
                                                           nf.value * nb.value), None, "animations")
            out.append({"name": name.value.decode(), "frame_rate": rate.value, "frames": m})
        return out

    def add_node(self, mesh, xf16=None):
        arr = None
        if xf16 is not None:
            arr = (C.c_float * 16)(*[float(x) for x in xf16])
        r = self._L.ctl_host_scene_add_node(self._h, mesh, arr)
        if r < 0:
            _check(1, None, "add_node")
        return r

    def add_area_light(self, node, local_material, radiance):
        """DiffuseLight on material `local_material` of `node`.  The nodes of a mesh share its materials:
        compile() refuses a mesh that carries a light and has more than one node."""
        arr = (C.c_float * 3)(*radiance)
        r = self._L.ctl_host_scene_add_area_light(self._h, node, local_material, arr)
        if r < 0:
            _check(1, None, "add_area_light")
        return r

    def add_point_light(self, pos, intensity):
        """PointLight(pos, intensity); returns its light index in the next compile (delta lights follow
        the area lights and the environment, in the order they were added)."""
        f3 = C.c_float * 3
        r = self._L.ctl_host_scene_add_point_light(self._h, f3(*pos), f3(*intensity))
        if r < 0:
            _check(1, None, "add_point_light")
        return r

    def add_spot_light(self, pos, target, intensity, cutoff_deg, beam_deg):
        """SpotLight(pos, target, intensity, width=cutoff_deg, fall=beam_deg): full intensity inside the
        beam width, a linear-in-angle fall to zero at the cutoff angle; returns its light index."""
        f3 = C.c_float * 3
        r = self._L.ctl_host_scene_add_spot_light(self._h, f3(*pos), f3(*target), f3(*intensity), float(cutoff_deg),
                                                  float(beam_deg))
        if r < 0:
            _check(1, None, "add_spot_light")
        return r

    def add_distant_light(self, irradiance, direction, scene_radius):
        """DistantLight(irradiance, direction.normalized(), scene_radius): the light travels along
        `direction`.  As in the reference, its disk is centred at direction * 1.1 * scene_radius about
        the origin, and only points on or beyond the disk's plane are lit;
        returns its light index."""
        f3 = C.c_float * 3
        r = self._L.ctl_host_scene_add_distant_light(self._h, f3(*irradiance), f3(*direction), float(scene_radius))
        if r < 0:
            _check(1, None, "add_distant_light")
        return r

    def add_homogeneous_volume(self, to_world, sigma_a, sigma_s, phase="isotropic", g=0.0, le=(0, 0, 0)):
        """HomogeneousVolumeDensity(phase function, to_world, sigma_a, sigma_s, le): a medium filling the
        unit cube transformed by the row-major 4x4 `to_world`; phase is "isotropic" or "hg" (Henyey-Greenstein
        with |g| < 1).  A scene holds one volume at most; returns its index (0)."""
        phases = {"isotropic": _abi.CTL_PHASE_ISOTROPIC, "hg": _abi.CTL_PHASE_HG}
        if phase not in phases:
            raise ValueError(f"add_homogeneous_volume: phase must be one of {sorted(phases)}")
        f3 = C.c_float * 3
        m = (C.c_float * 16)(*np.asarray(to_world, dtype=np.float32).reshape(16))
        r = self._L.ctl_host_scene_add_homogeneous_volume(self._h, m, f3(*sigma_a), f3(*sigma_s), f3(*le),
                                                          phases[phase], float(g))
        if r < 0:
            _check(1, None, "add_homogeneous_volume")
        return r

    def set_camera(self, pos, target, up, fov_deg, width, height, near=1.0, far=100000.0):
        f3 = C.c_float * 3
        _check(self._L.ctl_host_scene_set_camera(self._h, f3(*pos), f3(*target), f3(*up), fov_deg, near, far,
                                                  width, height), None, "set_camera")

    def set_sensor(self, kind, aperture_radius=0.0, focus_distance=None, screen_scale=(1, 1)):
        """Which of the reference's five sensors the scene is seen through: kind is "perspective", "thinlens",
        "orthographic", "telecentric" or "spherical" (SENSOR_KINDS); called after set_camera, whose position, fov,
        near / far and resolution it keeps.  focus_distance is needed by "thinlens" and "telecentric".  On a compiled
        scene the description (self.desc) takes the new camera and sensor records at once: hand it to
        Tracer.update_scene(desc, 0), no recompile."""
        if kind not in SENSOR_KINDS:
            raise ValueError(f"set_sensor: kind must be one of {sorted(SENSOR_KINDS)}")
        focus = 0.0 if focus_distance is None else float(focus_distance)
        _check(self._L.ctl_host_scene_set_sensor(self._h, SENSOR_KINDS[kind], float(aperture_radius), focus,
                                                  (C.c_float * 2)(*[float(x) for x in screen_scale])), None, "set_sensor")
        if getattr(self, "desc", None) is not None:
            self._sensor = _abi.Sensor()   # owned here: the description points at it
            _check(self._L.ctl_host_scene_sensor_state(self._h, C.byref(self.desc.camera), C.byref(self._sensor)), None,
                   "sensor_state")
            self.desc.sensor = C.pointer(self._sensor)
        return self

    def set_flags(self, flags):
        _check(self._L.ctl_host_scene_set_flags(self._h, flags), None, "set_flags")

    def set_environment(self, texture, scale=(1.0, 1.0, 1.0)):
        """DynamicScene::setEnvironementMap: an InfiniteLight over image texture
        `texture` (an add_texture index) with radiance `scale`; None removes it."""
        tex = 0xFFFFFFFF if texture is None else int(texture)
        _check(self._L.ctl_host_scene_set_environment(self._h, tex, (C.c_float * 3)(*scale)), None,
               "set_environment")
        return self

    def set_environment_transform(self, rot):
        """InfiniteLight::m_worldTransform (Light.h:307): a 3x3 rotation, world = rot @ local."""
        r = np.ascontiguousarray(rot, dtype=np.float32).reshape(9)
        _check(self._L.ctl_host_scene_set_environment_transform(self._h, (C.c_float * 9)(*r.tolist())), None,
               "set_environment_transform")
        return self

    def set_bvh_params(self, split_alpha=None, split_depth=8, bins=0, max_leaf=0):
        """BVH build knobs: reference splitting of large triangles (split_alpha = 0
        disables, None = library default), SAH bins per axis and max leaf size
        (0 = library default)."""
        if split_alpha is None:
            split_alpha = _abi.CTL_DEFAULT_SPLIT_ALPHA
        _check(self._L.ctl_host_scene_set_bvh_params(self._h, float(split_alpha), int(split_depth), int(bins),
                                                      int(max_leaf)), None, "set_bvh_params")
        return self

    def set_bvh_builder(self, builder="sbvh", split_alpha=1.0e-5):
        """Mesh BVH builder: "sbvh" (the reference's SplitBVHBuilder with in-build
        spatial splits, default) or "binned" (early split clipping + binned SAH)."""
        b = {"binned": _abi.CTL_BVH_BINNED, "sbvh": _abi.CTL_BVH_SBVH}[builder]
        _check(self._L.ctl_host_scene_set_bvh_builder(self._h, b, float(split_alpha)), None, "set_bvh_builder")
        return self

    def compile(self, threads=0):
        d = SceneDesc()
        _check(self._L.ctl_host_scene_compile(self._h, threads, C.byref(d)), None, "ctl_host_scene_compile")
        self.desc = d
        return d


def animation_frame_index(frame_rate, n_frames, t):
    """(frame, lerp) of AnimatedMesh::ComputeFrameIndex (ctl_animation_frame_index)."""
    frame, lerp = C.c_uint32(0), C.c_float(0.0)
    _check(lib().ctl_animation_frame_index(int(frame_rate), int(n_frames), float(t), C.byref(frame), C.byref(lerp)),
           None, "ctl_animation_frame_index")
    return frame.value, lerp.value


def woop_set(v0, v1, v2):
    """TriIntersectorData::setData (ctl_woop_set) per triangle: v0, v1, v2 = (n, 3) float32
    vertices (or one triangle's); returns the (n, 12) float32 Woop records."""
    a = np.ascontiguousarray(v0, dtype=np.float32).reshape(-1, 3)
    b = np.ascontiguousarray(v1, dtype=np.float32).reshape(-1, 3)
    c = np.ascontiguousarray(v2, dtype=np.float32).reshape(-1, 3)
    out = np.zeros((a.shape[0], 12), np.float32)
    f = lib().ctl_woop_set
    w = _abi.WoopTri()
    pa, pb, pc, stride = a.ctypes.data, b.ctypes.data, c.ctypes.data, 12
    for i in range(a.shape[0]):
        f(pa + stride * i, pb + stride * i, pc + stride * i, C.byref(w))
        out[i] = w.v[:]
    return out


def bvh_stack_bound(nodes, root_value=0):
    """(binary, 4-wide) worst-case traversal stack of a reference BVHNodeData
    tree (ctl_host_bvh_stack_bound); nodes = ctypes array / pointer of BVHNode."""
    out = (C.c_int32 * 2)()
    n = len(nodes)
    st = lib().ctl_host_bvh_stack_bound(C.cast(nodes, C.c_void_p), n, int(root_value), out)
    if st != 0:
        raise CTLError("ctl_host_bvh_stack_bound: " + (lib().ctl_host_last_error() or b"").decode())
    return out[0], out[1]


def host_wide_trees(desc):
    """The 4-wide trees ctl_scene_upload builds from desc (ctl_host_wide_trees):
    (mesh nodes (n, 32) float32, per-mesh first node (n_meshes,) uint32,
    instance-tree nodes (m, 32) float32), 128-B WideNode records as float32 rows
    (the child / pad words keep their int bits)."""
    L = lib()
    nm, ns = C.c_uint64(0), C.c_uint64(0)
    _check(L.ctl_host_wide_trees(C.byref(desc), None, 0, C.byref(nm), None, None, 0, C.byref(ns)), None,
           "ctl_host_wide_trees: " + (L.ctl_host_last_error() or b"").decode())
    mesh = np.zeros((nm.value, 32), np.float32)
    wbase = np.zeros(desc.n_meshes, np.uint32)
    scene = np.zeros((ns.value, 32), np.float32)
    _check(L.ctl_host_wide_trees(C.byref(desc), mesh.ctypes.data, nm.value, C.byref(nm), wbase.ctypes.data,
                                 scene.ctypes.data, ns.value, C.byref(ns)), None,
           "ctl_host_wide_trees: " + (L.ctl_host_last_error() or b"").decode())
    return mesh, wbase, scene


# ctl_block_info (VarianceBlockSampler::TmpBlockInfo) as a numpy record
BLOCK_INFO_DTYPE = np.dtype([("block_var_i", np.float32), ("num_pixels_var", np.uint32), ("block_e_i", np.float32),
                             ("block_e_i2", np.float32), ("num_pixels_e", np.uint32)])


class BlockSampler:
    """IBlockSampler (Kernel/BlockSampler/IBlockSampler.h): which blocks the next pass
    renders.  type "uniform" (UniformBlockSampler) or "variance" (VarianceBlockSampler:
    uniform for 10 passes, then the noisiest N / frac_weighted blocks plus every
    frac_deterministic-th one, rotating).  Host only, no GPU."""

    def __init__(self, width, height, tile_size=64, type="variance"):
        self._L = lib()
        t = {"uniform": _abi.CTL_BST_UNIFORM, "variance": _abi.CTL_BST_VARIANCE}.get(type, type)
        self._h = self._L.ctl_block_sampler_create(int(width), int(height), int(tile_size), int(t))
        if not self._h:
            self._h = None
            _check(1, None, "ctl_block_sampler_create")
        self.width, self.height, self.tile_size = int(width), int(height), int(tile_size)
        self.blocks_x = -(-self.width // self.tile_size)
        self.blocks_y = -(-self.height // self.tile_size)
        self.num_blocks = self.blocks_x * self.blocks_y

    def close(self):
        if getattr(self, "_h", None):
            self._L.ctl_block_sampler_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def start_new_rendering(self):
        _check(self._L.ctl_block_sampler_start_new_rendering(self._h), None, "ctl_block_sampler_start_new_rendering")

    def set_fractions(self, frac_deterministic=2, frac_weighted=4):
        _check(self._L.ctl_block_sampler_set_fractions(self._h, int(frac_deterministic), int(frac_weighted)), None,
               "ctl_block_sampler_set_fractions")

    def set_user_weight(self, bx, by, w):
        _check(self._L.ctl_block_sampler_set_user_weight(self._h, int(bx), int(by), float(w)), None,
               "ctl_block_sampler_set_user_weight")

    def blocks(self):
        """IterateBlocks: the block ids of the next pass, in order (uint32 array)."""
        n = C.c_uint32(0)
        out = np.zeros(2 * self.num_blocks, np.uint32)   # a block is listed twice at most (once per half)
        _check(self._L.ctl_block_sampler_blocks(self._h, out.ctypes.data, out.size, C.byref(n)), None,
               "ctl_block_sampler_blocks")
        return out[:n.value].copy()

    def tile_samples(self):
        """The next pass's list as one uint8 count per block (variance_add_pass's tile_samples)."""
        out = np.zeros(self.num_blocks, np.uint8)
        _check(self._L.ctl_block_sampler_tile_samples(self._h, out.ctypes.data), None,
               "ctl_block_sampler_tile_samples")
        return out

    def add_pass(self, info=None):
        """AddPass: `info` = the finished pass's block statistics (BLOCK_INFO_DTYPE records or
        anything of that layout, one per block); the uniform sampler needs none."""
        if info is None:
            _check(self._L.ctl_block_sampler_add_pass(self._h, None, 0), None, "ctl_block_sampler_add_pass")
            return
        a = np.ascontiguousarray(info)
        if a.dtype != BLOCK_INFO_DTYPE:
            a = np.ascontiguousarray(a).view(np.uint8).reshape(-1).view(BLOCK_INFO_DTYPE)
        _check(self._L.ctl_block_sampler_add_pass(self._h, a.ctypes.data, a.size), None, "ctl_block_sampler_add_pass")

    def weights(self):
        out = np.zeros(self.num_blocks, np.float32)
        _check(self._L.ctl_block_sampler_weights(self._h, out.ctypes.data), None, "ctl_block_sampler_weights")
        return out

    def passes_done(self):
        out = np.zeros(self.num_blocks, np.uint32)
        _check(self._L.ctl_block_sampler_passes_done(self._h, out.ctypes.data), None, "ctl_block_sampler_passes_done")
        return out


class Tracer:
    """Per-GPU traversal context (InitializeKernel/UpdateKernel/IntersectBuffers)."""

    def __init__(self, device=0):
        self._L = lib()
        self._ctx = self._L.ctl_create(int(device))
        if not self._ctx:
            raise CTLError("ctl_create failed: " + (self._L.ctl_last_error(None) or b"").decode())
        self.device = device

    def close(self):
        if self._ctx:
            self._L.ctl_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload_scene(self, desc):
        _check(self._L.ctl_scene_upload(self._ctx, C.byref(desc)), self._ctx, "ctl_scene_upload")

    def update_scene(self, desc, dirty=0, stream=0):
        """UpdateKernel / DynamicScene::UpdateScene (ctl_scene_update): the scene constants
        always, plus the array groups in `dirty` (_abi.CTL_DIRTY_*)."""
        _check(self._L.ctl_scene_update(self._ctx, C.byref(desc), int(dirty), stream), self._ctx, "ctl_scene_update")

    def set_transform(self, node, xf16, stream=0):
        """DynamicScene::SetNodeTransform on the device (ctl_scene_set_transform):
        xf16 = row-major object->world 4x4."""
        m = _abi.Float4x4()
        m.m[:] = [float(x) for x in np.asarray(xf16, dtype=np.float32).reshape(16)]
        _check(self._L.ctl_scene_set_transform(self._ctx, int(node), C.byref(m), stream), self._ctx,
               "ctl_scene_set_transform")

    def generate_samples(self, pass_index, stream=0):
        _check(self._L.ctl_sampler_generate(self._ctx, int(pass_index), stream), self._ctx, "ctl_sampler_generate")

    def intersect_buffers(self, n, rays_ptr, hits_ptr, any_hit=False, stream=0):
        _check(self._L.ctl_intersect(self._ctx, int(n), rays_ptr, hits_ptr, 1 if any_hit else 0, stream),
               self._ctx, "ctl_intersect")

    def occluded(self, n, rays_ptr, out_ptr, any_hit=False, stream=0):
        """KernelDynamicScene::Occluded(ray, 0, ray.tmax) per ray into uint32 out
        (ctl_occluded): the reference's closest-hit form or the any-hit query."""
        _check(self._L.ctl_occluded(self._ctx, int(n), rays_ptr, out_ptr, 1 if any_hit else 0, stream),
               self._ctx, "ctl_occluded")

    def intersect_stats(self, n, rays_ptr, hits_ptr, any_hit=False, stream=0):
        out = (C.c_uint64 * 4)()
        _check(self._L.ctl_intersect_stats(self._ctx, int(n), rays_ptr, hits_ptr, 1 if any_hit else 0, out, stream),
               self._ctx, "ctl_intersect_stats")
        return list(out)

    def animate(self, anim, frame0, frame1, lerp, stream=0):
        """AnimatedMesh::k_ComputeState on the device: frame0/frame1 = (n_bones, 4, 4) bone matrices."""
        f0 = np.ascontiguousarray(frame0, dtype=np.float32).reshape(-1, 16)
        f1 = np.ascontiguousarray(frame1, dtype=np.float32).reshape(-1, 16)
        if f0.shape != f1.shape:
            raise ValueError("frames differ in bone count")
        _check(self._L.ctl_scene_animate(self._ctx, int(anim), f0.ctypes.data, f1.ctypes.data, f0.shape[0],
                                         float(lerp), stream), self._ctx, "ctl_scene_animate")

    def set_animation(self, anim, animation, frames, frame_rate=0):
        """Keeps animation `animation` of animated mesh `anim` on the device
        (ctl_scene_set_animation): frames = (n_frames, n_bones, 4, 4).  Call after upload_scene."""
        f = np.ascontiguousarray(frames, dtype=np.float32)
        if f.ndim != 4 or f.shape[2:] != (4, 4):
            raise ValueError("frames must be (n_frames, n_bones, 4, 4)")
        _check(self._L.ctl_scene_set_animation(self._ctx, int(anim), int(animation), f.ctypes.data, f.shape[0],
                                               f.shape[1]), self._ctx, "ctl_scene_set_animation")
        self._anim_rates = getattr(self, "_anim_rates", {})
        self._anim_rates[(int(anim), int(animation))] = int(frame_rate)

    def upload_animations(self, host_scene):
        """Every animation of every animated mesh of host_scene's last compile, made
        resident (set_animation); the scene must have been uploaded from that compile."""
        d = host_scene.desc
        if d is None:
            raise CTLError("upload_animations: compile the host scene first")
        for a in range(d.n_anim_meshes):
            for k, an in enumerate(host_scene.animations(d.anim_meshes[a].mesh)):
                self.set_animation(a, k, an["frames"], an["frame_rate"])

    def animate_frame(self, anim, animation, frame, lerp, stream=0):
        """AnimatedMesh::k_ComputeState(animation, frame, lerp) from the resident frames:
        skins between `frame` and (frame + 1) % n_frames."""
        _check(self._L.ctl_scene_animate_frame(self._ctx, int(anim), int(animation), int(frame), float(lerp), stream),
               self._ctx, "ctl_scene_animate_frame")

    def animate_time(self, anim, animation, t, frame_rate=None, stream=0):
        """animate_frame at time t (seconds): frame and lerp from ctl_animation_frame_index at
        the animation's frame rate (the one set_animation / upload_animations recorded)."""
        if frame_rate is None:
            frame_rate = getattr(self, "_anim_rates", {}).get((int(anim), int(animation)), 0)
        _check(self._L.ctl_scene_animate_time(self._ctx, int(anim), int(animation), int(frame_rate), float(t), stream),
               self._ctx, "ctl_scene_animate_time")

    def read_array(self, which, first, count, dtype, width):
        """Device scene array slice (ctl_scene_read) as a (count, width) numpy array."""
        out = np.zeros((count, width), dtype)
        _check(self._L.ctl_scene_read(self._ctx, int(which), int(first), int(count), out.ctypes.data), self._ctx,
               "ctl_scene_read")
        return out

    def array_size(self, which):
        """Elements the device currently holds of a read_array array (ctl_scene_array_size):
        the uploaded length plus, for the tree arrays, the regions rebuild_mesh appended."""
        n = C.c_uint64(0)
        _check(self._L.ctl_scene_array_size(self._ctx, int(which), C.byref(n)), self._ctx, "ctl_scene_array_size")
        return int(n.value)

    def rebuild_mesh(self, mesh, positions_ptr, n_tris, stream=0):
        """Mesh::CompileMesh + ConstructBVH for resident geometry (ctl_scene_rebuild_mesh): mesh
        `mesh`'s trees rebuilt on the device from positions_ptr = n_tris x 9 device floats
        (v0 v1 v2 per triangle, the mesh's triangle order, object space)."""
        _check(self._L.ctl_scene_rebuild_mesh(self._ctx, int(mesh), positions_ptr, int(n_tris), stream), self._ctx,
               "ctl_scene_rebuild_mesh")

    def last_rebuild_ms(self):
        """Host milliseconds of the last rebuild_mesh's two phases (ctl_last_rebuild_ms): until the
        build's first stream synchronisation, and from there to the end of the second."""
        ms = (C.c_float * 2)()
        _check(self._L.ctl_last_rebuild_ms(self._ctx, C.byref(ms)), self._ctx, "ctl_last_rebuild_ms")
        return float(ms[0]), float(ms[1])

    def wide_trees(self, desc):
        """The uploaded scene's 4-wide trees as the device holds them (after any
        refit by animate / set_transform), in host_wide_trees' layout; float
        nodes only (not CTL_SCENE_WIDE_QUANT)."""
        if desc.flags & _abi.CTL_SCENE_WIDE_QUANT:
            raise ValueError("wide_trees: quantized trees are read as host_wide_trees' decoded boxes")
        mesh0, wbase0, scene0 = host_wide_trees(desc)
        mesh = self.read_array(_abi.CTL_ARRAY_WIDE_BVH, 0, mesh0.shape[0], np.float32, 32)
        wbase = self.read_array(_abi.CTL_ARRAY_MESH_WIDE_BASE, 0, wbase0.size, np.uint32, 1).reshape(-1)
        scene = self.read_array(_abi.CTL_ARRAY_SCENE_WIDE_BVH, 0, scene0.shape[0], np.float32, 32)
        return mesh, wbase, scene

    def light_eval(self, n, queries_ptr, results_ptr, stream=0):
        """Light::sampleDirect of the uploaded scene's lights for n ctl_light_query records in device
        memory (ctl_light_eval); results to n ctl_light_result records in device memory."""
        _check(self._L.ctl_light_eval(self._ctx, int(queries_ptr), int(n), int(results_ptr), stream or None), self._ctx,
               "ctl_light_eval")

    def sensor_eval(self, n, queries_ptr, results_ptr, stream=0):
        """Sensor::sampleRay / sampleRayDifferential of the uploaded scene's sensor for n ctl_sensor_query records
        in device memory (ctl_sensor_eval); results to n ctl_sensor_result records in device memory."""
        _check(self._L.ctl_sensor_eval(self._ctx, int(queries_ptr), int(n), int(results_ptr), stream or None), self._ctx,
               "ctl_sensor_eval")

    def medium_eval(self, n, queries_ptr, results_ptr, stream=0):
        """The medium's five operations of the uploaded scene's volume for n ctl_medium_query records in
        device memory (ctl_medium_eval); results to n ctl_medium_result records in device memory."""
        _check(self._L.ctl_medium_eval(self._ctx, int(queries_ptr), int(n), int(results_ptr), stream or None), self._ctx,
               "ctl_medium_eval")

    def bsdf_eval(self, n, queries_ptr, results_ptr, stream=0):
        """BSDFALL::sample / f / pdf of the uploaded scene's materials for n ctl_bsdf_query records in
        device memory (ctl_bsdf_eval); results to n ctl_bsdf_result records in device memory."""
        _check(self._L.ctl_bsdf_eval(self._ctx, int(n), int(queries_ptr), int(results_ptr), stream or None), self._ctx,
               "ctl_bsdf_eval")

    def math_eval(self, fn, n, a_ptr, b_ptr, out_ptr, stream=0):
        """The scalar arithmetic of the kernels for n elements in device memory (ctl_math_eval): `fn` as
        host_math_eval's; a_ptr / b_ptr to 32-bit input words (b_ptr 0 for a one-argument function),
        out_ptr to the uint32 result words."""
        _check(self._L.ctl_math_eval(self._ctx, _math_fn(fn), int(n), int(a_ptr), int(b_ptr) or None, int(out_ptr),
                                     stream or None), self._ctx, "ctl_math_eval")

    def rays_traced(self):
        return int(self._L.ctl_rays_traced(self._ctx))

    def tail_handovers(self):
        """(lanes, breaks) of the persistent path kernels' tail hand-over since the last reset_rays
        (ctl_tail_handovers): unfinished traversals carried over to a wave's next iteration, and the
        trace loops left early to do so."""
        lanes, breaks = C.c_uint64(0), C.c_uint64(0)
        _check(self._L.ctl_tail_handovers(self._ctx, C.byref(lanes), C.byref(breaks)), self._ctx, "ctl_tail_handovers")
        return int(lanes.value), int(breaks.value)

    def reset_rays(self, stream=0):
        _check(self._L.ctl_reset_rays(self._ctx, stream), self._ctx, "ctl_reset_rays")

    def image_resolve(self, fb_ptr, width, height, out_ptr, splat_scale=0.0, stream=0):
        """applyImagePipeline without filter/post-process: RGBA8 sRGB output (ImagePipeline.cu)."""
        _check(self._L.ctl_image_resolve(self._ctx, fb_ptr, width, height, float(splat_scale), out_ptr, stream),
               self._ctx, "ctl_image_resolve")

    def image_pipeline(self, fb_ptr, width, height, out_ptr, filter=None, tonemap=None, var_ptr=None,
                       filtered_ptr=None, splat_scale=0.0, num_passes=0, stream=0):
        """applyImagePipeline (ctl_image_pipeline): `filter` an ImageFilter (image_filter(...)) or None,
        `tonemap` a Tonemap or None; RGBA8 into out_ptr, the filtered RGBE image into filtered_ptr when
        given.  CTL_FILTER_NLM needs var_ptr (PixelVariance records) and keeps its weights in the
        context between calls with consecutive num_passes (update_periodicity)."""
        _check(self._L.ctl_image_pipeline(self._ctx, fb_ptr, var_ptr, int(width), int(height), float(splat_scale),
                                          int(num_passes), C.byref(filter) if filter is not None else None,
                                          C.byref(tonemap) if tonemap is not None else None, filtered_ptr, out_ptr,
                                          stream), self._ctx, "ctl_image_pipeline")

    def image_luminance(self, rgbe_ptr, width, height, stream=0):
        """Image::ComputeLuminanceInfo of a device RGBE image (ctl_image_luminance) as a LuminanceInfo;
        fixed summation order, so bitwise reproducible.  Synchronises."""
        out = LuminanceInfo()
        _check(self._L.ctl_image_luminance(self._ctx, rgbe_ptr, int(width), int(height), C.byref(out), stream),
               self._ctx, "ctl_image_luminance")
        return out

    def variance_add_pass(self, fb_ptr, width, height, tile_samples, var_ptr, splat_scale=0.0, tile_size=64,
                          stream=0):
        """PixelVarianceBuffer::AddPass; tile_samples = uint8 samples per tile this pass."""
        flags = np.ascontiguousarray(tile_samples, dtype=np.uint8)
        _check(self._L.ctl_variance_add_pass(self._ctx, fb_ptr, width, height, float(splat_scale), int(tile_size),
                                             flags.ctypes.data, var_ptr, stream), self._ctx, "ctl_variance_add_pass")

    def variance_stats(self, var_ptr, n, err_ptr=None, variance_ptr=None, average_ptr=None, stream=0):
        _check(self._L.ctl_variance_stats(self._ctx, var_ptr, int(n), err_ptr, variance_ptr, average_ptr, stream),
               self._ctx, "ctl_variance_stats")

    def block_stats(self, var_ptr, width, height, tile_size, out_ptr, stream=0):
        """VarianceBlockSampler's updateInfo (ctl_block_stats): the per-block sums of the pixel
        variances and averages into device ctl_block_info[ceil(w/ts) * ceil(h/ts)] (20 B each,
        BLOCK_INFO_DTYPE), summed in a fixed order -- bitwise reproducible."""
        _check(self._L.ctl_block_stats(self._ctx, var_ptr, int(width), int(height), int(tile_size), out_ptr, stream),
               self._ctx, "ctl_block_stats")

    def sync(self, stream=0):
        """Wait for the stream; raises CTLError if a traversal stack overflowed since the last reset_rays."""
        _check(self._L.ctl_sync(self._ctx, stream), self._ctx, "ctl_sync")

    def stack_bound(self):
        """Worst-case traversal stack (entries per lane) of the uploaded scene."""
        return int(self._L.ctl_scene_stack_bound(self._ctx))

    def fb_reduce(self, comm, fb_ptr, out_ptr, n_pixels, root=0, stream=0):
        """Sum every rank's PixelData framebuffer fb into out on the root (ctl_fb_reduce
        over an RCCL communicator from comm_init_all / comm_init_rank or the caller's);
        fb is only read, so it may be called after any step."""
        _check(self._L.ctl_fb_reduce(self._ctx, comm, fb_ptr, out_ptr, int(n_pixels), int(root), stream), self._ctx,
               "ctl_fb_reduce")


def comm_unique_id():
    """ncclGetUniqueId bytes (ctl_comm_unique_id) for comm_init_rank on every rank."""
    buf = (C.c_uint8 * CTL_COMM_ID_BYTES)()
    if lib().ctl_comm_unique_id(buf) != 0:
        raise CTLError("ctl_comm_unique_id failed")
    return bytes(buf)


def comm_init_rank(nranks, uid, rank, device):
    """One RCCL communicator of a one-process-per-GPU job (ctl_comm_init_rank)."""
    out = C.c_void_p()
    buf = (C.c_uint8 * CTL_COMM_ID_BYTES).from_buffer_copy(uid)
    if lib().ctl_comm_init_rank(C.byref(out), int(nranks), buf, int(rank), int(device)) != 0:
        raise CTLError("ctl_comm_init_rank failed")
    return out.value


def comm_init_all(devices):
    """RCCL communicators of one process driving `devices` (ctl_comm_init_all)."""
    n = len(devices)
    out = (C.c_void_p * n)()
    devs = (C.c_int32 * n)(*devices)
    if lib().ctl_comm_init_all(out, n, devs) != 0:
        raise CTLError("ctl_comm_init_all failed")
    return list(out)


def comm_destroy(comm):
    if lib().ctl_comm_destroy(comm) != 0:
        raise CTLError("ctl_comm_destroy failed")


class PathTracer(Tracer):
    """PathTracer (Integrators/PathTracer.h:7-24) parameters and pass loop.
    Defaults: Direct=1, MaxPathLength=50, RRStartDepth=5 (PathTracer.h:16-19)."""

    def __init__(self, device=0, max_path_length=50, rr_start_depth=5, shadow_any_hit=True, tile_size=64,
                 num_ranks=1, rank=0, schedule="persistent"):
        """schedule: "persistent" (regenerating path kernel, default), "megakernel"
        (one thread per pixel path) or "wavefront"; all bit-identical."""
        super().__init__(device)
        flags = {"persistent": 0, "megakernel": CTL_PT_MEGAKERNEL, "wavefront": CTL_PT_WAVEFRONT}[schedule]
        self.params = PTParams(1, max_path_length, rr_start_depth, 1 if shadow_any_hit else 0, tile_size,
                               num_ranks, rank, flags)

    def do_pass(self, fb_ptr, pass_index, stream=0):
        """UpdateKernel's sampler regeneration + one render pass into fb (device PixelData[w*h])."""
        self.generate_samples(pass_index, stream)
        _check(self._L.ctl_render_pass(self._ctx, C.byref(self.params), fb_ptr, stream), self._ctx,
               "ctl_render_pass")

    def render_pass(self, fb_ptr, stream=0):
        """One pass with the sampler tables already generated (generate_samples)."""
        _check(self._L.ctl_render_pass(self._ctx, C.byref(self.params), fb_ptr, stream), self._ctx,
               "ctl_render_pass")

    def render_passes(self, fb_ptr, first_pass, n_passes, stream=0):
        """Passes first_pass .. first_pass + n_passes - 1 in one launch (ctl_render_passes):
        the framebuffer of n_passes do_pass calls."""
        _check(self._L.ctl_render_passes(self._ctx, C.byref(self.params), int(first_pass), int(n_passes), fb_ptr,
                                         stream), self._ctx, "ctl_render_passes")

    def last_pass_ms(self):
        """Device time of the last render pass (Tracer::getLastTimeSpentRenderingSec)."""
        ms = C.c_float()
        _check(self._L.ctl_last_pass_ms(self._ctx, C.byref(ms)), self._ctx, "ctl_last_pass_ms")
        return ms.value

    def camera_rays(self, rays_ptr=None, capacity=0, stream=0):
        """Primary rays of the current pass (sampler tables from generate_samples) as a
        ctl_ray batch; returns the ray count (call with rays_ptr=None to query it)."""
        n = C.c_int64()
        _check(self._L.ctl_camera_rays(self._ctx, C.byref(self.params), rays_ptr, int(capacity), C.byref(n), stream),
               self._ctx, "ctl_camera_rays")
        return n.value

    def render_pass_blocks(self, fb_ptr, blocks, stream=0):
        """One pass over the listed blocks (ctl_render_pass_blocks) with the sampler tables
        already generated: a full pass masked to `blocks` (row-major block ids over
        params.tile_size blocks; an id listed m times is added m times)."""
        b = np.ascontiguousarray(blocks, dtype=np.uint32).reshape(-1)
        _check(self._L.ctl_render_pass_blocks(self._ctx, C.byref(self.params), b.ctypes.data if b.size else None,
                                              b.size, fb_ptr, stream), self._ctx, "ctl_render_pass_blocks")

    def do_pass_adaptive(self, fb_ptr, var_ptr, sampler, pass_index, stream=0):
        """Tracer<true>::DoPass with an IBlockSampler (Kernel/Tracer.h:209-248): the sampler
        tables of `pass_index`, a pass over sampler.blocks(), PixelVarianceBuffer::AddPass with
        the sampler's counts (splat scale 1 / passes), the per-block statistics, their
        read-back (20 B per block) and sampler.add_pass.  fb_ptr / var_ptr: device
        PixelData[w*h] / PixelVarianceInfo[w*h] (zeroed before the first pass).
        Returns the list that was rendered."""
        import torch
        if sampler.tile_size != (self.params.tile_size or 64):
            raise ValueError("do_pass_adaptive: the sampler's tile_size differs from params.tile_size")
        w, h, n = sampler.width, sampler.height, sampler.num_blocks
        blocks = sampler.blocks()
        counts = sampler.tile_samples()
        self.generate_samples(pass_index, stream)
        self.render_pass_blocks(fb_ptr, blocks, stream)
        self.variance_add_pass(fb_ptr, w, h, counts, var_ptr, splat_scale=1.0 / (pass_index + 1),
                               tile_size=sampler.tile_size, stream=stream)
        buf = getattr(self, "_block_info", None)
        if buf is None or buf.numel() < 5 * n:
            buf = self._block_info = torch.empty(5 * n, dtype=torch.int32, device=torch.device("cuda", self.device))
        self.block_stats(var_ptr, w, h, sampler.tile_size, buf.data_ptr(), stream)
        self.sync(stream)
        sampler.add_pass(buf[:5 * n].cpu().numpy().view(BLOCK_INFO_DTYPE))
        return blocks

    def pass_stats(self, fb_ptr, pass_index, stream=0):
        self.generate_samples(pass_index, stream)
        out = (C.c_uint64 * 4)()
        _check(self._L.ctl_render_pass_stats(self._ctx, C.byref(self.params), fb_ptr, out, stream), self._ctx,
               "ctl_render_pass_stats")
        return list(out)


class WavefrontPathTracer(Tracer):
    """WavefrontPathTracer (Integrators/PseudoRealtime/WavefrontPathTracer.h:24-67): path
    tracing over a DoubleRayBuffer, the batch traversal's second caller.  Defaults
    Direct=1, MaxPathLength=50, RRStartDepth=5 (WavefrontPathTracer.h:32-37)."""

    def __init__(self, device=0, direct=True, max_path_length=50, rr_start_depth=5, shadow_any_hit=False):
        super().__init__(device)
        self.params = WptParams(1 if direct else 0, max_path_length, rr_start_depth, 0,
                                _abi.CTL_WPT_SHADOW_ANY_HIT if shadow_any_hit else 0)
        self.passes_done = 0

    def do_pass(self, fb_ptr, pass_index, new_trace=False, stream=0):
        """Tracer::DoPass (Kernel/Tracer.h:209-248): UpdateKernel's sampler tables of
        `pass_index`, m_uPassesDone++ (reset by new_trace), then DoRender into fb."""
        if new_trace:
            self.passes_done = 0
        self.generate_samples(pass_index, stream)
        self.passes_done += 1
        self.params.passes_done = self.passes_done
        _check(self._L.ctl_wpt_render_pass(self._ctx, C.byref(self.params), fb_ptr, stream), self._ctx,
               "ctl_wpt_render_pass")

    def last_pass_ms(self):
        ms = C.c_float()
        _check(self._L.ctl_last_pass_ms(self._ctx, C.byref(ms)), self._ctx, "ctl_last_pass_ms")
        return ms.value


class PrimTracer(Tracer):
    """PrimTracer (Integrators/PrimTracer.h:11-22): one primary ray per pixel and
    a first-hit draw mode (default first_f, PrimTracer.cu:246), non-progressive
    (every pass clears the image, Tracer<false>::DoPass)."""

    def __init__(self, device=0, draw_mode="first_f", max_path_length=7, near=1.0, far=100000.0):
        super().__init__(device)
        mode = _abi.PRIM_DRAW_MODES.index(draw_mode) if isinstance(draw_mode, str) else int(draw_mode)
        self.params = _abi.PrimParams(mode, max_path_length, near, far, 0)

    def do_pass(self, fb_ptr, pass_index, depth_ptr=None, stream=0):
        """UpdateKernel's sampler regeneration + DoRender into fb (device PixelData[w*h]);
        depth_ptr: optional device float[w*h] for the D3D-normalised depth image."""
        self.generate_samples(pass_index, stream)
        _check(self._L.ctl_prim_pass(self._ctx, C.byref(self.params), fb_ptr, depth_ptr, stream), self._ctx,
               "ctl_prim_pass")

    def last_pass_ms(self):
        ms = C.c_float()
        _check(self._L.ctl_last_pass_ms(self._ctx, C.byref(ms)), self._ctx, "ctl_last_pass_ms")
        return ms.value

