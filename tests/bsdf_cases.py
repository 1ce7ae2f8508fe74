"""Materials, directed queries and the float32 restatement's answers for the batch BSDF entry
(ctl_host_bsdf_eval on the CPU, ctl_bsdf_eval on the GPU): shared by tests/test_bsdf_host.py and
tests/test_gpu_materials.py, computed once per process."""
import functools

import numpy as np

import bsdf_ref as R
import cudatracerlib_amd as ctl
from cudatracerlib_amd import _abi

f32 = np.float32
GOLD_ETA, GOLD_K = (0.143, 0.375, 1.442), (3.983, 2.386, 1.603)
ALU_ETA, ALU_K = (1.657, 0.880, 0.521), (9.224, 6.270, 4.837)

QUAD_V = [[-1, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1]]
QUAD_I = [[0, 2, 1], [0, 3, 2]]


def _d(type, two_sided=False, Rr=(1, 1, 1), T=(1, 1, 1), eta=1.5, **kw):
    d = dict(type=type, two_sided=two_sided, R=Rr, T=T, eta=eta, nonlinear=False)
    d.update(kw)
    return d


def _plastic(eta, diffuse, specular, nonlinear, two_sided):
    m, e = ctl.plastic_material(eta, diffuse, specular, nonlinear=nonlinear, two_sided=two_sided)
    return (m, e), _d(R.PLASTIC, two_sided, diffuse, (0, 0, 0), eta, specular=specular, fdr_int=e.fdr_int,
                      inv_eta2=e.inv_eta2, ssw=e.specular_sampling_weight, nonlinear=nonlinear)


@functools.lru_cache(maxsize=None)
def materials():
    """-> (list for HostScene.add_mesh, list of bsdf_ref dicts or None, by material index)."""
    A, D = [], []

    def add(a, d):
        A.append(a)
        D.append(d)

    add(ctl.diffuse_material(1.0, 1.0, 1.0, two_sided=False), None)                       # 0: the pinned warp
    rt = dict(Rr=(0.9, 0.8, 0.7), T=(0.6, 0.7, 0.95))
    for eta, ts in ((1.5, False), (1.0 / 1.5, False), (1.0, False), (1.5, True)):
        add(ctl.dielectric_material(eta, rt["Rr"], rt["T"], two_sided=ts), _d(R.DIELECTRIC, ts, eta=eta, **rt))
    for eta, ts in ((1.5, False), (0.75, False), (1.5, True)):
        add(ctl.thindielectric_material(eta, rt["Rr"], rt["T"], two_sided=ts), _d(R.THINDIELECTRIC, ts, eta=eta, **rt))
    for (e, k), ts in (((GOLD_ETA, GOLD_K), False), ((ALU_ETA, ALU_K), False), ((GOLD_ETA, GOLD_K), True)):
        add(ctl.conductor_material(e, k, (0.9, 0.95, 1.0), two_sided=ts),
            _d(R.CONDUCTOR, ts, (0.9, 0.95, 1.0), ext_eta=e, ext_k=k))
    for eta, nl, ts in ((1.5, False, False), (1.3, True, False), (1.5, False, True)):
        add(*_plastic(eta, (0.5, 0.3, 0.2), (1.0, 0.9, 0.8), nl, ts))
    # rough conductors and, with the same distributions, the rough dielectrics they are checked against
    for dist, alpha in ((_abi.CTL_MICROFACET_GGX, 0.3), (_abi.CTL_MICROFACET_BECKMANN, 0.25)):
        add(ctl.roughconductor_material(dist, GOLD_ETA, GOLD_K, alpha), dict(type=R.ROUGHCONDUCTOR, dist=dist, alpha=alpha))
    for dist, alpha in ((_abi.CTL_MICROFACET_GGX, 0.3), (_abi.CTL_MICROFACET_BECKMANN, 0.25)):
        add(ctl.roughdielectric_material(dist, 1.5, alpha), dict(type=5, dist=dist, alpha=alpha))
    # appended (the indices above stay): anisotropic rough conductors and a two-sided one
    for dist, au, av, ts in ((_abi.CTL_MICROFACET_GGX, 0.15, 0.4, False), (_abi.CTL_MICROFACET_BECKMANN, 0.35, 0.12, False),
                             (_abi.CTL_MICROFACET_GGX, 0.3, 0.2, True)):
        add(ctl.roughconductor_material(dist, ALU_ETA, ALU_K, au, av, (0.9, 0.95, 1.0), two_sided=ts),
            dict(type=R.ROUGHCONDUCTOR, dist=dist, alpha=au, alpha_v=av, two_sided=ts, appended=True))
    return A, D


def indices_of(type, appended=False):
    """Material indices of a type.  The materials appended later (anisotropic and two-sided rough
    conductors) are left out unless asked for: the property tests' bounds are derived for the first,
    isotropic pair."""
    return [i for i, d in enumerate(materials()[1])
            if d is not None and d["type"] == type and (appended or not d.get("appended"))]


@functools.lru_cache(maxsize=None)
def host_scene():
    hs = ctl.HostScene()
    A, _ = materials()
    mesh = hs.add_mesh(QUAD_V, QUAD_I, list(A), mat_index=[0, 0])
    hs.add_node(mesh)
    hs.set_camera((0, 3, 0.01), (0, 0, 0), (0, 1, 0), 40.0, 32, 32)
    return hs, hs.compile()


def _dir(cos, phi):
    s = np.sqrt(max(0.0, 1.0 - cos * cos))
    return np.array([s * np.cos(phi), s * np.sin(phi), cos], dtype=np.float64).astype(np.float32)


def _rot(v, ang):
    """v turned by ang about an axis perpendicular to it (float64, rounded once: an input)."""
    v = np.asarray(v, np.float64)
    v = v / np.linalg.norm(v)
    ax = np.cross(v, [0.3, -0.5, 0.81])
    ax /= np.linalg.norm(ax)
    return (v * np.cos(ang) + np.cross(ax, v) * np.sin(ang)).astype(np.float32)


COSINES = (1.0, 0.9, 0.5, 0.1, 1e-2, 1e-3, 1e-4)
LOBES = {R.DIELECTRIC: (R.EDELTA_REFLECTION, R.EDELTA_TRANSMISSION), R.THINDIELECTRIC: (R.EDELTA_REFLECTION, R.ENULL),
         R.CONDUCTOR: (R.EDELTA_REFLECTION, R.EGLOSSY_REFLECTION), R.PLASTIC: (R.EDELTA_REFLECTION, R.EDIFFUSE_REFLECTION)}


def _split(d, wi):
    """The Fresnel split sample.x is compared with, for wi as the lobe code sees it."""
    w = R.vec(wi)
    if w[2] < 0 and d["two_sided"]:
        w = (w[0], w[1], -w[2])
    with np.errstate(all="ignore"):
        if d["type"] == R.DIELECTRIC:
            return R.fresnel_dielectric_ext(w[2], R._eta_of(d)[0])[0]
        if d["type"] == R.THINDIELECTRIC:
            return R.thin_R(d, w)
        if d["type"] == R.PLASTIC:
            return R.plastic_prob_specular(d, R.fresnel_dielectric_ext(w[2], f32(d["eta"]))[0])
    return f32(0.5)


def _exact_wos(d, wi):
    """reflected, transmitted (refracted / passed through) directions of wi, as the lobe code forms them."""
    w = R.vec(wi)
    flip = w[2] < 0 and d["two_sided"]
    if flip:
        w = (w[0], w[1], -w[2])
    refl = R.reflect(w)
    with np.errstate(all="ignore"):
        if d["type"] == R.DIELECTRIC:
            eta, inv = R._eta_of(d)
            _, ct = R.fresnel_dielectric_ext(w[2], eta)
            tr = R.refract(w, ct, eta, inv)
        else:
            tr = R._neg(w)
    return [np.array(refl, np.float32), np.array(tr, np.float32)]


@functools.lru_cache(maxsize=None)
def delta_queries(type):
    """Directed queries for every material of a delta type (3, 4, 6, 8): BSDF_QUERY_DTYPE array."""
    _, D = materials()
    a, b = LOBES[type]
    masks = (a, b, a | b, 0, R.EALL)
    rows = []
    for mi in indices_of(type):
        d = D[mi]
        k = 0
        for cos in COSINES:
            for sign in (1.0, -1.0):
                k += 1
                wi = _dir(sign * cos, 0.37 + 0.9 * k)
                F = _split(d, wi)
                xs = [F, np.nextafter(F, f32(-1)), np.nextafter(F, f32(2)), f32(0.0), f32(0.5), f32(0.999)]
                for mask in masks:
                    for x in xs:
                        rows.append((mi, 0, mask, R.ESOLID_ANGLE, wi, (0, 0, 1), (x, 0.3), (0.5, 0.5)))
                refl, tr = _exact_wos(d, wi)
                # exact, inside DeltaEpsilon (1 - cos 0.03 = 4.5e-4), just past it (1 - cos 0.05 = 1.25e-3), unrelated
                wos = [refl, tr, _rot(refl, 0.03), _rot(refl, 0.05), _rot(tr, 0.05), _dir(0.6, 2.1)]
                for mask in masks:
                    for measure in (R.ESOLID_ANGLE, R.EDISCRETE):
                        for wo in wos:
                            for op in (1, 2):
                                rows.append((mi, op, mask, measure, wi, wo, (0, 0), (0.5, 0.5)))
    q = np.zeros(len(rows), dtype=ctl.BSDF_QUERY_DTYPE)
    for i, r in enumerate(rows):
        q[i] = r
    return q


@functools.lru_cache(maxsize=None)
def roughconductor_queries(n=4200):
    """sample / f / pdf queries over every rough conductor (the appended anisotropic and two-sided
    ones included): random directions, three quarters of them in the upper hemisphere, the masks
    EALL, glossy only and delta only, both measures.  BSDF_QUERY_DTYPE array."""
    rng = np.random.RandomState(3)
    rc = indices_of(R.ROUGHCONDUCTOR, appended=True)
    q = np.zeros(n, dtype=ctl.BSDF_QUERY_DTYPE)
    for i in range(len(q)):
        d = rng.normal(size=(2, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        if i % 4:
            d[:, 2] = np.abs(d[:, 2])
        mask = (R.EALL, R.EGLOSSY_REFLECTION, R.EDELTA_REFLECTION)[0 if i % 5 else (i // 5) % 3]
        q[i] = (rc[rng.randint(len(rc))], i % 3, mask, R.EDISCRETE if i % 11 == 0 else R.ESOLID_ANGLE, d[0], d[1],
                rng.uniform(0, 1, 2), (0.5, 0.5))
    return q


def pack(results):
    """bsdf_ref result tuples -> BSDF_RESULT_DTYPE array."""
    out = np.zeros(len(results), dtype=ctl.BSDF_RESULT_DTYPE)
    for i, (v, pdf, wo, st) in enumerate(results):
        out[i] = (v, pdf, wo, st)
    return out


def reference(q, warp=None):
    _, D = materials()
    return pack([R.bsdfall(D[int(r["material"])], int(r["op"]), r["wi"], r["wo"], int(r["type_mask"]), int(r["measure"]),
                           r["sample"], warp) for r in q])


def plastic_reference(q, evaluate):
    """The restatement's answers to plastic queries, with the cosine warp taken from `evaluate`'s
    diffuse material (index 0) at the remapped sample.  evaluate: queries -> BSDF_RESULT_DTYPE array.
    -> (results, number of distinct warps)."""
    _, D = materials()
    need = {}
    for r in q:
        if int(r["op"]) != 0:
            continue
        d = D[int(r["material"])]
        wi = R.vec(r["wi"])
        if wi[2] < 0 and d["two_sided"]:
            wi = (wi[0], wi[1], -wi[2])
        with np.errstate(all="ignore"):
            s = R.plastic_remap(d, wi, int(r["type_mask"]), r["sample"])
        if s is not None:
            need[(np.float32(s[0]).tobytes(), np.float32(s[1]).tobytes())] = s
    keys = list(need)
    wq = np.zeros(len(keys), dtype=ctl.BSDF_QUERY_DTYPE)
    for i, k in enumerate(keys):
        wq[i] = (0, 0, R.EALL, R.ESOLID_ANGLE, (0, 0, 1), (0, 0, 1), need[k], (0.5, 0.5))
    wres = evaluate(wq)
    table = {k: R.vec(wres[i]["wo"]) for i, k in enumerate(keys)}
    warp = lambda s: table[(np.float32(s[0]).tobytes(), np.float32(s[1]).tobytes())]   # noqa: E731
    return reference(q, warp), len(keys)


def same_bits(a, b):
    """Field-wise bit equality of two BSDF_RESULT_DTYPE arrays: the indices that differ.  A NaN equals
    a NaN (IEEE 754 fixes neither its sign nor its payload, and the processors differ): the float
    fields' NaNs are set to one pattern first.  sample.x = 0 puts the cosine warp on the disk's rim,
    where 1 - x^2 - y^2 rounds below zero and z is NaN."""
    def canon(r):
        v = np.frombuffer(r.tobytes(), np.uint32).reshape(-1, 8).copy()
        fl = v[:, :7].view(np.float32)
        v[:, :7][np.isnan(fl)] = 0x7fc00000
        return v
    return np.nonzero((canon(a) != canon(b)).any(axis=1))[0]
