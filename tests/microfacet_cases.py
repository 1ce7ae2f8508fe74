"""The rough dielectric and the rough conductor held to tests/microfacet_ref.py (float64, from the
papers): a scene of this file's own, the query sets, and the checks as functions of an `evaluate`
callable (BSDF_QUERY_DTYPE array -> BSDF_RESULT_DTYPE array).  tests/test_microfacet_host.py passes
ctl_host_bsdf_eval, tests/test_gpu_microfacet.py the HIP batch entry ctl_bsdf_eval; neither check
reads the other's results.  Everything that depends only on the reference (query arrays, expected bin
counts, conditioning) is computed once per process."""
import functools

import numpy as np

import microfacet_ref as M
import cudatracerlib_amd as ctl
from cudatracerlib_amd import _abi
from bsdf_cases import ALU_ETA, ALU_K, GOLD_ETA, GOLD_K, QUAD_I, QUAD_V

f32 = np.float32
U = 2.0 ** -24                 # one fp32 rounding, relative
ONE_M = f32(1.0 - 2.0 ** -24)  # the largest float below 1
EGR, EGT = _abi.CTL_EGLOSSY_REFLECTION, _abi.CTL_EGLOSSY_TRANSMISSION
BOTH = EGR | EGT
SOLID, DISCRETE = 1, 4
OP_SAMPLE, OP_F, OP_PDF = 0, 1, 2
BECK, GGX = _abi.CTL_MICROFACET_BECKMANN, _abi.CTL_MICROFACET_GGX

# kind, distribution, alpha_u, alpha_v, eta (dielectric) or (eta, k) (conductor), R, T, two_sided
_SPEC = [
    ("dielectric", GGX, 0.3, 0.3, 1.5, (0.9, 0.6, 0.75), (0.5, 0.85, 0.7), False),
    ("dielectric", BECK, 0.25, 0.25, 1.5, (0.8, 0.7, 0.55), (0.65, 0.9, 0.4), False),
    ("dielectric", GGX, 0.15, 0.4, 1.5, (0.7, 0.95, 0.6), (0.9, 0.45, 0.8), False),
    ("dielectric", BECK, 0.35, 0.12, 1.33, (0.6, 0.85, 0.95), (0.75, 0.55, 0.9), False),
    ("dielectric", GGX, 0.25, 0.25, 1.0 / 1.5, (0.95, 0.75, 0.5), (0.85, 0.6, 0.95), False),
    ("conductor", GGX, 0.3, 0.3, (GOLD_ETA, GOLD_K), (0.9, 0.95, 1.0), None, False),
    ("conductor", BECK, 0.35, 0.12, (ALU_ETA, ALU_K), (0.8, 0.9, 0.7), None, False),
    ("conductor", GGX, 0.3, 0.2, (GOLD_ETA, GOLD_K), (0.95, 0.85, 0.9), None, True),
]
N_MAT = len(_SPEC)            # materials N_MAT .. 2 N_MAT - 1: the same with R = T = 1
DIELECTRICS = [i for i, s in enumerate(_SPEC) if s[0] == "dielectric"]
CONDUCTORS = [i for i, s in enumerate(_SPEC) if s[0] == "conductor"]


@functools.lru_cache(maxsize=None)
def scene():
    """-> (HostScene, compiled description, list of microfacet_ref.Material by material index)."""
    A, refs = [], []
    for white in (False, True):
        for kind, dist, au, av, eta, R, T, ts in _SPEC:
            R_ = (1.0, 1.0, 1.0) if white else R
            T_ = (1.0, 1.0, 1.0) if white or T is None else T
            # what the product is given is float32: the reference gets the same numbers
            c = lambda v: tuple(float(f32(x)) for x in v)   # noqa: E731
            name = M.BECKMANN if dist == BECK else M.GGX
            if kind == "dielectric":
                A.append(ctl.roughdielectric_material(dist, eta, au, av, R_, T_))
                refs.append(M.Material(kind, name, float(f32(au)), float(f32(av)), eta=float(f32(eta)), R=c(R_), T=c(T_)))
            else:
                A.append(ctl.roughconductor_material(dist, eta[0], eta[1], au, av, R_, two_sided=ts))
                refs.append(M.Material(kind, name, float(f32(au)), float(f32(av)), eta=c(eta[0]), k=c(eta[1]), R=c(R_),
                                       two_sided=ts))
    hs = ctl.HostScene()
    hs.add_node(hs.add_mesh(QUAD_V, QUAD_I, A, mat_index=[0, 0]))
    hs.set_camera((0, 3, 0.01), (0, 0, 0), (0, 1, 0), 40.0, 32, 32)
    return hs, hs.compile(), refs


def host_evaluate(q):
    return ctl.host_bsdf_eval(scene()[1], q)


def queries(material, op, mask, measure, wi, wo=None, sample=None):
    n = len(wi)
    q = np.zeros(n, dtype=ctl.BSDF_QUERY_DTYPE)
    q["material"], q["op"], q["type_mask"], q["measure"] = material, op, mask, measure
    q["wi"] = wi
    q["wo"] = (0, 0, 1) if wo is None else wo
    if sample is not None:
        q["sample"] = sample
    q["uv"] = 0.5
    return q


def _dirs(rng, n, sign):
    """n directions with |z| uniform in [0.05, 1] and the sign(s) given, float64."""
    z = rng.uniform(0.05, 1.0, n) * sign
    return M.sphere_dirs(z, rng.uniform(0, 2 * np.pi, n))


# ---------------------------------------------------------------------------------------------
# Conditioning, from the reference alone.
#
# The product forms H = normalize(wi + eta wo) in fp32 (eta = 1 for reflection): the product eta wo
# and the sum round each component (absolute error at most u (eta + |v|), v the unnormalised sum),
# lenSqr and 1/len scale all components alike (no change of direction), and the final products round
# each component once more (u).  So H is off in direction by at most u (eta / |v| + 2).  The dot
# products wi.H and wo.H start from 0 and round three products and two sums of magnitude <= 1: an
# absolute error of 4u at most, the same as another 4u of direction.  Doubled for safety:
#     eps_H = 2u (eta / |v| + 2) + 4u                              (18u at eta = 1.5, |v| = 0.3)
# What this does to f and pdf is measured on the reference: H is nudged by eps_H along +-t1, +-t2 (two
# tangents) and the largest relative change is taken, times sqrt(2) for a nudge between the tangents.
# That covers D (condition 2E / (sin cos) in the Beckmann exponent E), the Fresnel term (unbounded at
# the critical angle, where cos_t^2 = 1 - sin^2 / eta^2 cancels), |wo.H| and the Jacobian's
# denominator.  The remaining operations are relative roundings of well-conditioned + - * / sqrt:
#     alpha = (a + a + a) * (1/3)           3, passed on by D with 2E + 2 <= 16 (D >= 1e-3 D(n))     48
#     D: squares, quotients, sum, exp, product of five                                           14
#     G1 twice (1 - z^2 is exact to u / 0.0025 at |z| <= 1: |z| >= 0.05; fit or hypot)           2 x 14
#     F given its cosine                                                                         12
#     the products and quotients of f or pdf                                                     14
#                                                                                         N_FIXED = 116
# A pair is well conditioned when  sqrt(2) max_nudge |f' / f - 1| + N_FIXED u <= BOUND = 1e-4.
N_FIXED = 116
BOUND = 1e-4


def conditioning(mat, wi, wo, lobes, extra_eps=0.0, chains=1, fixed=N_FIXED):
    """-> (bound on the relative fp32 error of f and of pdf per pair, by the derivation above; inf
    where the reference is 0).  H is nudged by eps_H + extra_eps; `chains` product computations with
    `fixed` well-conditioned roundings in all are compared (one, against the reference, by default)."""
    refl = wi[:, 2] * wo[:, 2] > 0
    n_i, n_o = M._sides(mat, wi) if mat.kind == "dielectric" else (np.ones(len(wi)), np.ones(len(wi)))
    eta = np.where(refl, 1.0, n_o / n_i)
    vlen = np.sqrt(M.dot(wi + eta[:, None] * wo, wi + eta[:, None] * wo))
    with np.errstate(all="ignore"):
        eps = 2 * U * (eta / vlen + 2) + 4 * U + extra_eps
    _, h, _, _ = M.geometry(mat, wi, wo)
    t1 = M.normalize(np.cross(h, np.array([0.37, -0.48, 0.8])))
    t2 = np.cross(h, t1)
    f0, p0 = M.f(mat, wi, wo, lobes)[:, 0], M.pdf(mat, wi, wo, lobes)
    worst = np.zeros(len(wi))
    with np.errstate(all="ignore"):
        for t in (t1, -t1, t2, -t2):
            dh = t * eps[:, None]
            worst = np.maximum(worst, np.abs(M.f(mat, wi, wo, lobes, dh=dh)[:, 0] / f0 - 1.0))
            worst = np.maximum(worst, np.abs(M.pdf(mat, wi, wo, lobes, dh=dh) / p0 - 1.0))
    b = chains * np.sqrt(2.0) * worst + fixed * U
    return np.where((f0 > 0) & (p0 > 0) & np.isfinite(b), b, np.inf), eta, vlen, h


def well_conditioned(mat, wi, wo, lobes, **kw):
    """The pairs the float64 reference alone declares well conditioned: the derived bound holds, and
    |wi + eta wo| >= 0.3, D(H) >= 1e-3 D(n), |wo.H| and |wi.H| >= 0.05, 1 - F >= 0.05 for
    transmission, F >= 1e-3 for reflection."""
    b, eta, vlen, h = conditioning(mat, wi, wo, lobes, **kw)
    refl = wi[:, 2] * wo[:, 2] > 0
    a = (mat.dist, mat.au, mat.av)
    keep = (b <= BOUND) & (vlen >= 0.3) & (M.D(*a, h) >= 1e-3 * M.D(*a, np.array([[0.0, 0.0, 1.0]])))
    keep &= (np.abs(M.dot(wo, h)) >= 0.05) & (np.abs(M.dot(wi, h)) >= 0.05)
    if mat.kind == "dielectric":
        n_i, n_o = M._sides(mat, wi)
        F = M.fresnel_dielectric(np.abs(M.dot(wi, h)), n_o / n_i)
        keep &= np.where(refl, F >= 1e-3, 1.0 - F >= 0.05)
    return keep


# ---------------------------------------------------------------------------------------------
# (a) closed forms
N_PAIRS = 20000


@functools.lru_cache(maxsize=None)
def closed_form_pairs(mi):
    """N_PAIRS (wi, wo) pairs for material mi, float32: wi on either side (above only for the
    conductors: below, a one-sided one is black and a two-sided one is the reference's BSDFALL
    wrapper, which flips wi alone before f and pdf), |z| down to 0.05.  wo is the mirror image or
    the refraction of wi about a microfacet normal drawn where D is not negligible (slopes in an
    ellipse of 2.4 alpha for Beckmann, 4 alpha for GGX), alternating, so that both lobes are
    populated; where that fails (total internal reflection, wo grazing or on the wrong side) wo is
    uniform on the lobe's hemisphere.  -> (wi, wo, is_reflection)"""
    mat = scene()[2][mi]
    rng = np.random.RandomState(100 + mi)
    n = N_PAIRS
    cond = mat.kind == "conductor"
    wi = _dirs(rng, n, 1.0 if cond else np.where(rng.uniform(size=n) < 0.5, 1.0, -1.0))
    r = np.sqrt(rng.uniform(size=n)) * (2.4 if mat.dist == M.BECKMANN else 4.0)
    ph = rng.uniform(0, 2 * np.pi, n)
    m = M.normalize(np.stack([-r * mat.au * np.cos(ph), -r * mat.av * np.sin(ph), np.ones(n)], axis=-1))
    want_refl = np.ones(n, bool) if cond else (np.arange(n) % 2 == 0)
    c = M.dot(wi, m)
    wo_r = 2 * c[:, None] * m - wi
    if cond:
        wo_t, ok_t = wo_r, np.zeros(n, bool)
    else:
        n_i, n_o = M._sides(mat, wi)
        e = n_i / n_o
        with np.errstate(all="ignore"):
            ct2 = 1 - e * e * (1 - c * c)
            wo_t = -e[:, None] * wi + (e * c - np.sign(c) * np.sqrt(np.maximum(ct2, 0)))[:, None] * m   # Snell
        ok_t = (ct2 > 0) & (wo_t[:, 2] * wi[:, 2] < 0) & (np.abs(wo_t[:, 2]) >= 0.05) & (c * wi[:, 2] > 0)
    ok_r = (wo_r[:, 2] * wi[:, 2] > 0) & (np.abs(wo_r[:, 2]) >= 0.05)
    sgn = np.sign(wi[:, 2]) * np.where(want_refl, 1.0, -1.0)
    fallback = _dirs(rng, n, sgn)
    wo = np.where(want_refl[:, None], np.where(ok_r[:, None], wo_r, fallback), np.where(ok_t[:, None], wo_t, fallback))
    wi, wo = wi.astype(f32), wo.astype(f32)
    return wi, wo, want_refl


def check_closed_forms(evaluate, mi):
    """ops f and pdf (two-lobe and single-lobe masks) against the reference on the well-conditioned
    pairs of material mi, within BOUND = 1e-4 relative (the derivation is above `conditioning`); the
    channels carry R or T as exact factors; zeros where the reference is zero.  -> dict of figures."""
    mat = scene()[2][mi]
    wi, wo, refl = closed_form_pairs(mi)
    wi64, wo64 = wi.astype(np.float64), wo.astype(np.float64)
    assert ((wi64[:, 2] * wo64[:, 2] > 0) == refl).all()
    single = np.where(refl, EGR, EGT).astype(np.uint32)
    full = EGR if mat.kind == "conductor" else BOTH
    f_all = evaluate(queries(mi, OP_F, full, SOLID, wi, wo))
    p_all = evaluate(queries(mi, OP_PDF, full, SOLID, wi, wo))
    p_one = evaluate(queries(mi, OP_PDF, single, SOLID, wi, wo))
    f_one = evaluate(queries(mi, OP_F, single, SOLID, wi, wo))
    lobes_all = M.REFLECTION if mat.kind == "conductor" else M.REFLECTION | M.TRANSMISSION
    keep = well_conditioned(mat, wi64, wo64, lobes_all)
    out = {}
    worst = 0.0
    for name, lobe in (("reflection", refl), ("transmission", ~refl)):
        if not lobe.any():
            continue
        k = keep & lobe
        share = k.sum() / lobe.sum()
        out[name + " kept"] = share
        assert share >= 0.25, (mi, name, share)
        want_f = M.f(mat, wi64[k], wo64[k], lobes_all)
        want_p2 = M.pdf(mat, wi64[k], wo64[k], lobes_all)
        want_p1 = M.pdf(mat, wi64[k], wo64[k], M.REFLECTION if name == "reflection" else M.TRANSMISSION)
        ef = np.abs(f_all["value"][k].astype(np.float64) / want_f - 1.0).max()
        ef1 = np.abs(f_one["value"][k].astype(np.float64) / want_f - 1.0).max()
        ep2 = np.abs(p_all["pdf"][k].astype(np.float64) / want_p2 - 1.0).max()
        ep1 = np.abs(p_one["pdf"][k].astype(np.float64) / want_p1 - 1.0).max()
        out[name] = dict(f=ef, pdf_two_lobe=ep2, pdf_one_lobe=ep1)
        worst = max(worst, ef, ef1, ep2, ep1)
        if mat.kind == "dielectric":   # R or T is a factor of every channel: fl(c_k v) / fl(c_0 v), two roundings
            col = mat.R if name == "reflection" else mat.T
            v = f_all["value"][k].astype(np.float64)
            ratio = np.abs((v / v[:, :1]) / (col / col[0]) - 1.0).max()
            out[name + " colour"] = ratio
            assert ratio <= 2 * U * (1 + 4 * U), (mi, name, ratio / U)
    out["worst"] = worst
    print(f"material {mi} closed forms: worst relative error {worst:.3g} (bound {BOUND:g}); {out}")
    assert worst <= BOUND, (mi, out)
    # zeros: the lobe not in the mask, the discrete measure, and for a conductor wo or wi below
    other = np.where(refl, EGT, EGR).astype(np.uint32)
    for op in (OP_F, OP_PDF):
        z = evaluate(queries(mi, op, other, SOLID, wi, wo))
        assert not z["value"].any() and not z["pdf"].any(), (mi, op, "lobe not in the mask")
        z = evaluate(queries(mi, op, full, DISCRETE, wi, wo))
        assert not z["value"].any() and not z["pdf"].any(), (mi, op, "discrete measure")
        z = evaluate(queries(mi, op, 0x1ff & ~BOTH, SOLID, wi, wo))
        assert not z["value"].any() and not z["pdf"].any(), (mi, op, "no glossy lobe in the mask")
        if mat.kind == "conductor":
            z = evaluate(queries(mi, op, full, SOLID, wi, wo * f32([1, 1, -1])))
            assert not z["value"].any() and not z["pdf"].any(), (mi, op, "wo below a conductor")
            if not mat.two_sided:
                z = evaluate(queries(mi, op, full, SOLID, -wi, -wo))
                assert not z["value"].any() and not z["pdf"].any(), (mi, op, "one-sided conductor from below")
            else:
                # BSDFALL::f / pdf (SceneTypes/BSDF.h:185-199) flip wi.z alone before the call and wi.z and
                # wo.z after it.  So from below, with wo above, a two-sided material answers as from above
                # (the values just held to the reference, bit for bit) and hands wo back mirrored; with wo
                # below as well it sees wo under the flipped wi and answers zero.
                down = f32([1, 1, -1])
                z = evaluate(queries(mi, op, full, SOLID, wi * down, wo))
                above = f_all if op == OP_F else p_all
                assert (z["value"].view(np.uint32) == above["value"].view(np.uint32)).all(), (mi, op, "two-sided, wi below")
                assert (z["pdf"].view(np.uint32) == above["pdf"].view(np.uint32)).all(), (mi, op, "two-sided, wi below")
                assert (z["wo"] == wo * down).all(), (mi, op, "two-sided: wo handed back mirrored")
                assert (above["value"] > 0).any() if op == OP_F else (above["pdf"] > 0).any()
                z = evaluate(queries(mi, op, full, SOLID, wi * down, wo * down))
                assert not z["value"].any() and not z["pdf"].any(), (mi, op, "two-sided, wi and wo below")
    if mat.kind == "conductor" and not mat.two_sided:
        s = evaluate(queries(mi, OP_SAMPLE, full, SOLID, -wi, sample=np.random.RandomState(5).uniform(0, 0.99, (len(wi), 2))))
        assert not s["value"].any() and not s["pdf"].any()
    return out


# ---------------------------------------------------------------------------------------------
# (b) the density of the samples
N_SAMPLES = 200000
BINS, SUB = 16, 24
AZIMUTH = 0.7   # off the axes and off the diagonals


def chi2_quantile(dof, p=1e-6):
    """The upper p quantile of chi-square with dof degrees of freedom: scipy's where scipy is
    installed, else Wilson-Hilferty, dof (1 - 2 / (9 dof) + z sqrt(2 / (9 dof)))^3 with z the normal
    quantile (4.753424 at p = 1e-6); against scipy's it is 2.9 % high at 8 degrees of freedom, 1.1 % at
    20, 0.4 % at 50 and 0.05 % at 256."""
    try:
        from scipy.stats import chi2
        return float(chi2.isf(p, dof))
    except ImportError:
        assert p == 1e-6
        return dof * (1 - 2 / (9 * dof) + 4.753424 * np.sqrt(2 / (9 * dof))) ** 3


def density_cases():
    """(material, wi.z, mask): the dielectrics from 0.8, 0.3 and -0.8 with each lobe alone, the
    conductors from 0.8 and 0.3."""
    out = [(mi, z, mask) for mi in DIELECTRICS for z in (0.8, 0.3, -0.8) for mask in (EGR, EGT)]
    return out + [(mi, z, EGR) for mi in CONDUCTORS for z in (0.8, 0.3)]


def _wi_of(z):
    return M.sphere_dirs(np.array([z]), np.array([AZIMUTH])).astype(f32)


def _cells(split):
    """The BINS x BINS bins of (|cos theta|, phi) as rectangles (c0, c1, p0, p1) with their bin index.
    A bin that contains |cos| = split is two rectangles: the transmission pdf jumps there for GGX
    (h.z = 0, where D stays finite and the half vector changes sides), and a rule that straddles a
    jump converges like 1 / nodes."""
    edges = np.arange(BINS + 1) / BINS
    if split is not None and 0 < split < 1 and np.abs(edges - split).min() > 1e-9:
        edges = np.sort(np.append(edges, split))
    cells, ids = [], []
    for a, b in zip(edges[:-1], edges[1:]):
        ci = min(int(0.5 * (a + b) * BINS), BINS - 1)
        for k in range(BINS):
            cells.append((a, b, -np.pi + k * 2 * np.pi / BINS, -np.pi + (k + 1) * 2 * np.pi / BINS))
            ids.append(ci * BINS + k)
    return np.array(cells), np.array(ids)


def _cell_integrals(fn, cells, sub, sign):
    """Integrals of fn(wo) over rectangles of (|cos theta|, phi), z = sign |cos|: tensor Gauss-Legendre, sub x sub nodes."""
    x, w = np.polynomial.legendre.leggauss(sub)
    c = 0.5 * (cells[:, 0] + cells[:, 1])[:, None] + 0.5 * (cells[:, 1] - cells[:, 0])[:, None] * x    # (k, sub)
    p = 0.5 * (cells[:, 2] + cells[:, 3])[:, None] + 0.5 * (cells[:, 3] - cells[:, 2])[:, None] * x
    C = np.repeat(c[:, :, None], sub, axis=2)
    P = np.repeat(p[:, None, :], sub, axis=1)
    v = np.asarray(fn(M.sphere_dirs(sign * C.ravel(), P.ravel())))
    several = v.ndim == 2                                     # fn may return k integrands as (N, k)
    v = v.reshape(len(cells), sub, sub, -1)
    area = 0.25 * (cells[:, 1] - cells[:, 0]) * (cells[:, 3] - cells[:, 2])
    out = (v * w[None, :, None, None] * w[None, None, :, None]).sum(axis=(1, 2)) * area[:, None]
    return out if several else out[:, 0]


def _bin_integrals(fn, sign, split):
    """-> (per-bin integrals, what the last doubling of the nodes moved each bin by, relative).
    SUB / 2 and SUB nodes per bin and dimension everywhere; the bins that this still moves by more
    than 0.05 % (kinks of the integrand: wi.h = 0, wo.h = 0) are doubled again, up to 8 SUB."""
    cells, ids = _cells(split)

    def bins(sub, which):
        sel = np.isin(ids, which)
        out = np.zeros(BINS * BINS)
        np.add.at(out, ids[sel], _cell_integrals(fn, cells[sel], sub, sign))
        return out[which]

    every = np.arange(BINS * BINS)
    prev, cur = bins(SUB // 2, every), bins(SUB, every)
    sub = SUB
    with np.errstate(all="ignore"):
        move = np.where(cur > 0, np.abs(prev / cur - 1.0), 0.0)
        while sub < 8 * SUB:
            bad = every[(move > 5e-4) & (cur * N_SAMPLES >= 1)]
            if not len(bad):
                break
            sub *= 2
            new = bins(sub, bad)
            move[bad] = np.where(new > 0, np.abs(cur[bad] / new - 1.0), 0.0)
            cur[bad] = new
    return cur.reshape(BINS, BINS), move.reshape(BINS, BINS)


@functools.lru_cache(maxsize=None)
def expected_bins(mi, z, mask):
    """-> (p_fit, move, p_exact): per-bin probabilities of wo under the reference pdf times
    [G1(wo, H) > 0]; what the last doubling of the quadrature moved each bin by (must be <= 0.1 % in
    every bin used); for Beckmann the same with the exact Smith G1, which is the density the
    visible-normal sampling draws from while pdf() (and so the expectation) uses Walter's fit."""
    mat = scene()[2][mi]
    wi = _wi_of(z).astype(np.float64)
    lobe = M.REFLECTION if mask == EGR else M.TRANSMISSION
    sign = np.sign(z) * (1.0 if mask == EGR else -1.0)
    split = None
    if mask == EGT:   # h.z = 0 where n_i wi.z + n_o wo.z = 0
        n_i, n_o = M._sides(mat, wi)
        split = float(n_i[0] / n_o[0] * abs(wi[0, 2]))

    def run(beck):
        fn = lambda wo: M.pdf(mat, np.broadcast_to(wi, wo.shape), wo, lobe, beckmann=beck, indicator=True)   # noqa: E731
        return _bin_integrals(fn, sign, split)

    p_fit, move = run("fit")
    p_exact = run("exact")[0] if mat.dist == M.BECKMANN else p_fit
    return p_fit, move, p_exact


def _categories(p, n):
    """The chi-square's categories, each expecting >= 100 of n samples: every bin that does on its
    own, and runs of neighbouring smaller bins.  The smaller bins are walked ring by ring of
    |cos theta| and by ascending phi within a ring, and a run is closed as soon as it expects >= 100;
    what is left over at the end (< 100) belongs to no category.  So the GGX tail and the grazing
    rings are tested as many local categories, not as one aggregate.
    -> (labels per bin, -1 for a bin in no category; number of categories)"""
    e = (p * n).ravel()
    labels = np.full(e.shape, -1)
    single = e >= 100
    k = int(single.sum())
    labels[single] = np.arange(k)
    run, acc = [], 0.0
    for b in np.nonzero(~single)[0]:
        run.append(b)
        acc += e[b]
        if acc >= 100:
            labels[run] = k
            k, run, acc = k + 1, [], 0.0
    return labels.reshape(p.shape), k


def _fold(v, labels, k):
    use = labels >= 0
    return np.bincount(labels[use], weights=v[use], minlength=k)


def density_plan(mi, z, mask):
    """-> (n, labels, number of categories, quantile, bias estimate): the number of samples by the
    reference alone.  200,000 unless the Beckmann fit's bias estimate n sum (p_exact - p_fit)^2 /
    p_fit over the categories reaches half the chi-square quantile; then the largest power of ten at
    which it does not (and there must be one)."""
    p_fit, move, p_exact = expected_bins(mi, z, mask)
    for n in (N_SAMPLES, 100000, 10000, 1000):
        labels, k = _categories(p_fit, n)
        a, b = _fold(p_fit, labels, k), _fold(p_exact, labels, k)
        q = chi2_quantile(k)
        lam = n * ((b - a) ** 2 / a).sum()
        if lam < 0.5 * q:
            return n, labels, k, q, lam
    raise AssertionError((mi, z, mask, "the fit's bias estimate stays above half the quantile down to n = 1000", lam, q))


@functools.lru_cache(maxsize=None)
def density_samples(n, seed):
    s = np.random.RandomState(seed).random_sample((n, 2)).astype(f32)
    return np.minimum(s, ONE_M)


def density_queries(mi, z, mask):
    n = density_plan(mi, z, mask)[0]
    return queries(mi, OP_SAMPLE, mask, SOLID, np.repeat(_wi_of(z), n, axis=0), sample=density_samples(n, 77))


def check_density(evaluate, mi, z, mask):
    """chi-square of the sampled wo against the reference's expected counts, below the p = 1e-6
    quantile for the number of categories; the accepted share against the reference's integral within
    4 sigma.  The categories (_categories) each expect >= 100 samples: the bins that do on their own
    and runs of neighbouring smaller bins; together they must hold >= 99 % of the reference's mass
    (asserted on the categories alone; the single bins' own share is in the figures).  The share is
    compared with the integral under the exact Smith G1: that, not Walter's fit, is what the sampling
    inverts (for GGX the two are the same), and the fit's integral is printed beside it.  -> figures."""
    p_fit, move, p_exact = expected_bins(mi, z, mask)
    n, labels, dof, quant, lam = density_plan(mi, z, mask)
    mass, mass_exact = p_fit.sum(), p_exact.sum()
    cat_p = _fold(p_fit, labels, dof)
    assert (cat_p * n >= 100).all()
    quad = float((_fold(move * p_fit, labels, dof) / cat_p).max())   # what the last doubling moved a category by, at most
    assert quad <= 1e-3, (mi, z, mask, "quadrature", quad)
    held = cat_p.sum() / mass
    singles = p_fit[p_fit * n >= 100].sum() / mass
    assert held >= 0.99, (mi, z, mask, "the categories hold", held)
    exp = cat_p * n
    r = evaluate(density_queries(mi, z, mask))
    wo = r["wo"].astype(np.float64)
    sign = np.sign(z) * (1.0 if mask == EGR else -1.0)
    ok = (r["pdf"] > 0) & (r["value"].max(axis=1) > 0)
    assert np.isfinite(wo[ok]).all() and (wo[ok][:, 2] * sign > 0).all()
    assert (r["sampled_type"][ok] == mask).all()
    ci = np.minimum((np.abs(wo[ok][:, 2]) * BINS).astype(int), BINS - 1)
    pi = np.minimum(((np.arctan2(wo[ok][:, 1], wo[ok][:, 0]) + np.pi) * (BINS / (2 * np.pi))).astype(int), BINS - 1)
    counts = np.zeros((BINS, BINS))
    np.add.at(counts, (ci, pi), 1.0)
    obs = _fold(counts, labels, dof)
    chi = float(((obs - exp) ** 2 / exp).sum())
    share = ok.sum() / n
    m1 = min(mass_exact, 1.0)
    sigma = np.sqrt(m1 * (1 - m1) / n)
    quad_mass = max(float((move * p_fit).sum()), 1e-6)   # the quadrature's error in the total, 1e-6 at the least
    fig = dict(n=n, chi2=chi, dof=dof, quantile=quant, fit_bias_estimate=lam, share=share, reference_mass=mass_exact,
               fit_mass=mass, sigma=sigma, quadrature=quad, categories_hold=held, single_bins_hold=singles)
    print(f"material {mi} wi.z {z} mask {mask:#x}: chi2 {chi:.1f} at {dof} categories ({int((p_fit * n >= 100).sum())} single bins "
          f"holding {singles:.2%}, all {held:.3%}), quantile {quant:.1f}, n {n}, fit bias estimate {lam:.1f}; accepted {share:.5f}, "
          f"reference {mass_exact:.5f} (with the fit {mass:.5f}), sigma {sigma:.2g}; quadrature {quad:.1g}")
    if chi >= quant:
        b = (obs - exp) / np.sqrt(exp)
        print("per category (observed - expected) / sqrt(expected):\n", np.round(b, 1), "\nlabels:\n", labels)
    assert chi < quant, fig
    assert abs(share - mass_exact) <= 4 * sigma + quad_mass, fig
    return fig


# ---------------------------------------------------------------------------------------------
# (c) sample against f and pdf
N_IDENT = 20000


@functools.lru_cache(maxsize=None)
def identity_inputs(mi):
    mat = scene()[2][mi]
    rng = np.random.RandomState(300 + mi)
    up = mat.kind == "conductor"
    wi = _dirs(rng, N_IDENT, 1.0 if up else np.where(rng.uniform(size=N_IDENT) < 0.5, 1.0, -1.0)).astype(f32)
    s = np.minimum(rng.random_sample((N_IDENT, 2)).astype(f32), ONE_M)
    return wi, s


def check_sample_identities(evaluate, mi):
    """At the wo that op sample returns: its pdf equals op pdf, weight * pdf equals op f, for the
    single-lobe masks and for the two-lobe mask; sampled_type names the lobe; |wo| = 1 within 4u.

    Roundings.  sample computes D, G1, F and the Jacobian at the microfacet normal m, f and pdf at
    H = normalize(wi + eta wo) with wo = reflect(wi, m) or normalize(refract(wi, m)).  wo is off by
    at most 16u in direction for reflect (dot 5, 2 dot, times m, minus wi, normalize 8) and
    (4 + 3 (1 + eta))u < 12u for refract (the dot's 4u, then product, sum, product and difference
    of magnitude <= 1 + eta; normalize changes no direction beyond its final u), which H passes on
    times eta / |v|; H's own roundings are eps_H of `conditioning`.  So m and H differ by
        eps = eps_H + 16u eta / |v|,
    and what that does to f and pdf is measured on the reference as in `conditioning`; the fixed
    roundings count twice (two chains, each off by its own eps at most) plus the product
    weight * pdf: 2 N_FIXED + 1.  The samples kept are those with |wo.z| >= 0.05 that the reference
    declares well conditioned (`well_conditioned`) with the bound so derived <= BOUND = 1e-4; at least
    a quarter of the accepted samples must be among them."""
    mat = scene()[2][mi]
    wi, s = identity_inputs(mi)
    masks = (EGR,) if mat.kind == "conductor" else (EGR, EGT, BOTH)
    worst = dict(pdf=0.0, weight=0.0, length=0.0)
    for mask in masks:
        r = evaluate(queries(mi, OP_SAMPLE, mask, SOLID, wi, sample=s))
        ok = (r["pdf"] > 0) & (r["value"].max(axis=1) > 0)
        assert np.isfinite(r["wo"][ok]).all() and np.isfinite(r["value"]).all() and np.isfinite(r["pdf"]).all()
        st = r["sampled_type"][ok]
        wo = r["wo"][ok]
        same_side = wi[ok][:, 2] * wo[:, 2] > 0
        assert (np.where(same_side, EGR, EGT) == st).all() and ((st & mask) == st).all()
        if mask == BOTH:
            assert (st == EGR).sum() > 100 and (st == EGT).sum() > 100
        ln = np.abs(np.sqrt((wo.astype(np.float64) ** 2).sum(axis=1)) - 1.0).max()
        worst["length"] = max(worst["length"], ln)
        assert ln <= 4 * U, (mi, mask, ln / U)
        fr = evaluate(queries(mi, OP_F, mask, SOLID, wi[ok], wo))
        pr = evaluate(queries(mi, OP_PDF, mask, SOLID, wi[ok], wo))
        wi64, wo64 = wi[ok].astype(np.float64), wo.astype(np.float64)
        lobes = (M.REFLECTION if mask == EGR else M.TRANSMISSION) if mask != BOTH else M.REFLECTION | M.TRANSMISSION
        refl = wi64[:, 2] * wo64[:, 2] > 0
        n_i, n_o = M._sides(mat, wi64) if mat.kind == "dielectric" else (1.0, 1.0)
        eta = np.where(refl, 1.0, n_o / n_i)
        vlen = np.sqrt(((wi64 + eta[:, None] * wo64) ** 2).sum(axis=1))
        with np.errstate(all="ignore"):
            keep = well_conditioned(mat, wi64, wo64, lobes, extra_eps=16 * U * eta / vlen, chains=2, fixed=2 * N_FIXED + 1)
        keep &= np.abs(wo64[:, 2]) >= 0.05
        assert keep.sum() >= 0.25 * ok.sum(), (mi, mask, keep.sum(), ok.sum())
        sp, pp = r["pdf"][ok][keep].astype(np.float64), pr["pdf"][keep].astype(np.float64)
        w, fv = r["value"][ok][keep].astype(np.float64), fr["value"][keep].astype(np.float64)
        assert (pp > 0).all() and (fv > 0).all()
        e_p = np.abs(sp / pp - 1.0).max()
        e_w = np.abs(w * sp[:, None] / fv - 1.0).max()
        worst["pdf"], worst["weight"] = max(worst["pdf"], e_p), max(worst["weight"], e_w)
    print(f"material {mi} sample identities: pdf worst {worst['pdf']:.3g}, weight * pdf / f worst {worst['weight']:.3g} "
          f"(bound {BOUND:g}), |wo| - 1 worst {worst['length'] / U:.2f} roundings")
    assert worst["pdf"] <= BOUND and worst["weight"] <= BOUND, (mi, worst)
    return worst


# ---------------------------------------------------------------------------------------------
# (e) edge inputs
def edge_inputs():
    """wi x sample.x x sample.y -> (wi, sample) float32 arrays."""
    z9 = f32(0.99999)
    zs = [f32(1.0), np.nextafter(z9, f32(0)), z9, np.nextafter(z9, f32(2)), f32(1e-3)]
    wis = []
    for z in zs:
        for sgn in (1.0, -1.0):
            z64 = float(z)
            s = np.sqrt(max(0.0, 1.0 - z64 * z64))
            wis.append((s * np.cos(AZIMUTH), s * np.sin(AZIMUTH), sgn * z64))
    sx = [f32(0.0), f32(2.0 ** -24), f32(0.1), ONE_M]
    sy = [f32(0.0), f32(0.5), np.nextafter(f32(0.5), f32(1)), ONE_M]
    rows = [(w, (x, y)) for w in wis for x in sx for y in sy]
    return np.array([r[0] for r in rows], f32), np.array([r[1] for r in rows], f32)


def edge_queries():
    wi, s = edge_inputs()
    out = []
    for mi in range(2 * N_MAT):
        for mask in ((EGR,) if scene()[2][mi].kind == "conductor" else (EGR, EGT, BOTH)):
            out.append(queries(mi, OP_SAMPLE, mask, SOLID, wi, sample=s))
    return np.concatenate(out)


def check_edges(evaluate):
    """Every material at the edge inputs: finite, non-negative results of sample and of f and pdf at
    the sampled wo, and a weight of at most 1 + 8u where R = T = 1 and only reflection is asked for
    (the weight is F G1 <= 1; F's last operations, 0.5 (Rs^2 + Rp^2), the conductor's (Rp2 + Rs2) 0.5
    and R F, G1's quotient and the product: 8 roundings).  -> the sample results."""
    q = edge_queries()
    r = evaluate(q)
    bad = ~(np.isfinite(r["value"]).all(axis=1) & np.isfinite(r["pdf"]) & np.isfinite(r["wo"]).all(axis=1))
    assert not bad.any(), ("not finite", int(bad.sum()), q[bad][:5], r[bad][:5])
    assert (r["value"] >= 0).all() and (r["pdf"] >= 0).all()
    white = (q["material"] >= N_MAT) & (q["type_mask"] == EGR)
    wmax = float(r["value"][white].max())
    print(f"edge inputs: {len(q)} sample queries, largest reflection-only weight at R = 1: 1 + {(wmax - 1) / U:.2f} roundings")
    assert wmax <= 1 + 8 * U, wmax
    for op in (OP_F, OP_PDF):
        q2 = q.copy()
        q2["op"], q2["wo"] = op, r["wo"]
        r2 = evaluate(q2)
        bad = ~(np.isfinite(r2["value"]).all(axis=1) & np.isfinite(r2["pdf"]))
        assert not bad.any(), ("not finite", op, int(bad.sum()), q2[bad][:5], r2[bad][:5])
        assert (r2["value"] >= 0).all() and (r2["pdf"] >= 0).all()
    return r


# ---------------------------------------------------------------------------------------------
# (d) the reference's two deviations from the textbook, pinned as such
def check_lobe_choice(evaluate, mi, z, n=100000):
    """roughdielectric::sample with both lobes in the mask (SceneTypes/BSDF_Simple.cu:548-556) draws
    the microfacet normal m from sample.x and then picks the lobe from the same number, quantised:
    MonteCarlo::sampleReuse(10, sample.x, slot) (Math/MonteCarlo.cu:16-20) gives slot =
    floor(10 sample.x), and transmission is taken exactly when slot / 10 > F(wi.m).  So the lobe is
    neither independent of m nor chosen with probability F.  Pinned here per sample: m is recovered in
    float64 from the reflection-only query of the same (wi, sample), m = normalize(wi + wo); samples
    with |F - slot / 10| < 1e-4 are left out (under 1 %, asserted).  -> (reflection share, mean F, m's F)"""
    mat = scene()[2][mi]
    wi = np.repeat(_wi_of(z), n, axis=0)
    s = density_samples(n, 91)
    r1 = evaluate(queries(mi, OP_SAMPLE, EGR, SOLID, wi, sample=s))
    r2 = evaluate(queries(mi, OP_SAMPLE, BOTH, SOLID, wi, sample=s))
    valid = (r1["sampled_type"] == EGR) & np.isfinite(r1["wo"]).all(axis=1)
    assert valid.mean() > 0.999 and ((r2["sampled_type"] == EGR) | (r2["sampled_type"] == EGT))[valid].all()
    wi64 = wi.astype(np.float64)
    m = M.upper(M.normalize(wi64 + r1["wo"].astype(np.float64)))
    n_i, n_o = M._sides(mat, wi64)
    F = M.fresnel_dielectric(np.abs(M.dot(wi64, m)), n_o / n_i)
    slot = np.floor(s[:, 0] * f32(10)).astype(np.float64)      # the product's float32 product, as the reference's
    near = np.abs(F - slot / 10) < 1e-4
    assert near[valid].mean() < 0.01
    use = valid & ~near
    want_T = (slot / 10 > F)
    got_T = r2["sampled_type"] == EGT
    assert (want_T == got_T)[use].all(), (mi, z, int((want_T != got_T)[use].sum()))
    # the same normal is used by both queries: where the two-lobe query reflects, wo is the reflection-only query's
    both_R = use & ~got_T
    assert (r2["wo"][both_R] == r1["wo"][both_R]).all()
    share = 1.0 - got_T[use].mean()
    print(f"material {mi} wi.z {z}: two-lobe reflection share {share:.4f}, mean F {F[use].mean():.4f}, "
          f"{near[valid].mean():.2%} of the samples left out")
    return share, F[use], use.sum()


def check_lobe_share_is_a_step(evaluate, mi, z):
    """Where F(wi.m) stays inside one slot (k / 10, (k + 1) / 10] for nearly every sampled m, the
    reflection share is the step 0.1 (k + 1) = 0.1 ceil(10 F), not F: within 4 sigma of the binomial
    plus the share of samples whose F falls into another slot; and it is not the mean F by 10 sigma."""
    share, F, n = check_lobe_choice(evaluate, mi, z)
    mat = scene()[2][mi]
    wi = _wi_of(z).astype(np.float64)
    n_i, n_o = M._sides(mat, wi)
    step = np.ceil(10 * M.fresnel_dielectric(np.abs(wi[:, 2]), n_o / n_i)[0]) / 10
    outside = (np.ceil(10 * F) / 10 != step).mean()
    sigma = np.sqrt(step * (1 - step) / n)
    print(f"material {mi} wi.z {z}: step {step:.1f}, share {share:.4f}, {outside:.2%} of the samples in another slot, sigma {sigma:.2g}")
    assert outside < 0.05
    assert abs(share - step) <= 4 * sigma + outside, (share, step, outside)
    assert abs(share - F.mean()) > 10 * sigma, (share, F.mean())


def check_pdf_without_side_check(evaluate, mi, z):
    """roughdielectric::pdf (SceneTypes/BSDF_Simple.cu:373-435) does not ask whether wo lies on the
    valid side of the half vector for the transmission lobe; f does, through G (:485), and sample
    through its weight's G1(wo, m) (:600-601).  So the integral of op pdf over the transmission
    hemisphere exceeds the share of accepted samples, and with the reference's indicator
    [G1(wo, H) > 0] multiplied in it equals that share (4 sigma plus the quadrature's error, which is
    what doubling its nodes moves).  The integrand is the product's own pdf at the quadrature nodes."""
    mat = scene()[2][mi]
    wi = _wi_of(z)
    wi64 = wi.astype(np.float64)
    n_i, n_o = M._sides(mat, wi64)
    sign = -np.sign(z)
    cells, _ = _cells(float(n_i[0] / n_o[0] * abs(wi64[0, 2])))
    tot = {}
    def integrands(wo):
        """The product's pdf, and the same times the reference's indicator, at the same nodes."""
        pdf = evaluate(queries(mi, OP_PDF, EGT, SOLID, np.repeat(wi, len(wo), axis=0), wo.astype(f32)))["pdf"].astype(np.float64)
        ind = M.pdf(mat, np.broadcast_to(wi64, wo.shape), wo, M.TRANSMISSION, indicator=True) > 0
        return np.stack([pdf, pdf * ind], axis=1)

    tot = {sub: tuple(_cell_integrals(integrands, cells, sub, sign).sum(axis=0)) for sub in (SUB // 2, SUB)}
    plain, inside = tot[SUB]
    q_plain, q_inside = abs(plain - tot[SUB // 2][0]), abs(inside - tot[SUB // 2][1])
    r = evaluate(density_queries(mi, z, EGT))
    n = len(r)
    share = ((r["pdf"] > 0) & (r["value"].max(axis=1) > 0)).sum() / n
    sigma = np.sqrt(min(share, 1 - share + 1.0 / n) * max(share, 1.0 / n) / n)
    print(f"material {mi} wi.z {z}: integral of pdf over the transmission hemisphere {plain:.4f} (quadrature {q_plain:.1g}), "
          f"with [G1(wo, H) > 0] {inside:.4f} (quadrature {q_inside:.1g}), accepted share {share:.4f}, sigma {sigma:.2g}")
    assert plain - share > 4 * sigma + q_plain + 0.01, (plain, share)
    assert abs(inside - share) <= 4 * sigma + q_inside + 1e-4, (inside, share)
    return plain, inside, share


def check_two_sided_mirror(evaluate):
    """BSDFALL::sample (SceneTypes/BSDF.h:170-176) flips wi.z before and wi.z and wo.z after a
    two-sided material's sample: from below, the two-sided conductor returns the sample from above
    with wo.z negated, bit for bit."""
    mi = [i for i in CONDUCTORS if scene()[2][i].two_sided][0]
    wi, s = identity_inputs(mi)
    a = evaluate(queries(mi, OP_SAMPLE, EGR, SOLID, wi, sample=s))
    b = evaluate(queries(mi, OP_SAMPLE, EGR, SOLID, wi * f32([1, 1, -1]), sample=s))
    assert (a["value"] > 0).any()
    assert (a["value"].view(np.uint32) == b["value"].view(np.uint32)).all() and (a["pdf"].view(np.uint32) == b["pdf"].view(np.uint32)).all()
    ok = a["pdf"] > 0
    assert (a["wo"][ok] * f32([1, 1, -1]) == b["wo"][ok]).all() and (a["sampled_type"] == b["sampled_type"]).all()
