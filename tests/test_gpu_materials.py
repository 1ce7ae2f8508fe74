"""dielectric, thindielectric, conductor, roughconductor and plastic on the GPU: the batch BSDF
entry against its host twin, what upload accepts and refuses, the three PathTracer schedules, the
WavefrontPathTracer and the PrimTracer on a scene with all five types, and three renders whose
pixels are known in closed form (invisible panes, a mirror, a one-colour texture)."""
import ctypes as C

import numpy as np
import pytest
import torch

import bsdf_cases as BC
import bsdf_ref as R
import oracle
from helpers import binary_bvh, jitter_landing, oracle_render

U = 2.0 ** -24
ENV_RGB = (200, 180, 160)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def uniform_env(s, ctl):
    """A one-colour environment map (bilinear lookups of it differ only by rounding)."""
    img = np.full((8, 16), ENV_RGB[0] | (ENV_RGB[1] << 8) | (ENV_RGB[2] << 16) | (255 << 24), np.uint32)
    s.set_environment(s.add_texture(img, filter=ctl._abi.CTL_TEX_BILINEAR), (1.0, 1.0, 1.0))


class Mesh:
    def __init__(self):
        self.v, self.i, self.m, self.uv = [], [], [], []

    def quad(self, p, k):
        b = len(self.v)
        self.v.extend(p)
        self.uv.extend([(0, 0), (1, 0), (1, 1), (0, 1)])
        self.i.extend([(b, b + 1, b + 2), (b, b + 2, b + 3)])
        self.m.extend([k, k])

    def add_to(self, s, mats):
        return s.add_mesh(np.array(self.v, np.float32), np.array(self.i, np.uint32), mats,
                          mat_index=np.array(self.m, np.uint8), uvs=np.array(self.uv, np.float32))


def render(ctl, desc, params, passes, w, h, dev, batched=False):
    pt = ctl.PathTracer(0)
    try:
        pt.upload_scene(desc)
        pt.params = params
        fb = torch.zeros((w * h, 7), dtype=torch.float32, device=dev)
        if batched:
            pt.render_passes(fb.data_ptr(), 0, passes)
        else:
            for p in range(passes):
                pt.do_pass(fb.data_ptr(), p)
        torch.cuda.synchronize()
        return fb.cpu().numpy()
    finally:
        pt.close()


def same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_batch_entry_equals_the_host_entry_bit_for_bit(ctl, dev):
    """ctl_bsdf_eval (HIP) against ctl_host_bsdf_eval on the directed query sets of the four delta
    types (>= 4000 each) and on sample / f / pdf queries of the rough conductors."""
    _, desc = BC.host_scene()
    rng = np.random.RandomState(3)
    sets = {t: BC.delta_queries(t) for t in (R.DIELECTRIC, R.THINDIELECTRIC, R.CONDUCTOR, R.PLASTIC)}
    rc = BC.indices_of(R.ROUGHCONDUCTOR)
    q = np.zeros(4200, dtype=ctl.BSDF_QUERY_DTYPE)
    for i in range(len(q)):
        d = rng.normal(size=(2, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        if i % 4:
            d[:, 2] = np.abs(d[:, 2])
        mask = (R.EALL, R.EGLOSSY_REFLECTION, R.EDELTA_REFLECTION)[0 if i % 5 else (i // 5) % 3]
        q[i] = (rc[i % 2], i % 3, mask, R.EDISCRETE if i % 11 == 0 else R.ESOLID_ANGLE, d[0], d[1], rng.uniform(0, 1, 2),
                (0.5, 0.5))
    sets[R.ROUGHCONDUCTOR] = q
    t = ctl.Tracer(0)
    try:
        t.upload_scene(desc)
        for type, qs in sets.items():
            assert len(qs) >= 4000
            dq = torch.from_numpy(np.frombuffer(qs.tobytes(), np.uint8).copy()).to(dev)
            dr = torch.zeros(len(qs) * 32, dtype=torch.uint8, device=dev)
            t.bsdf_eval(len(qs), dq.data_ptr(), dr.data_ptr())
            torch.cuda.synchronize()
            got = np.frombuffer(dr.cpu().numpy().tobytes(), dtype=ctl.BSDF_RESULT_DTYPE)
            want = ctl.host_bsdf_eval(desc, qs)
            bad = BC.same_bits(got, want)
            assert bad.size == 0, (type, len(bad), qs[bad[0]], got[bad[0]], want[bad[0]])
            assert (want["value"].max(axis=1) > 0).sum() > len(qs) // 20
    finally:
        t.close()


def _one_material_scene(ctl, mat, texture=False):
    s = ctl.HostScene()
    if texture:
        s.add_texture(np.full((4, 4), 0xff808080, np.uint32))
    m = Mesh()
    m.quad([(-1, 0, -1), (-1, 0, 1), (1, 0, 1), (1, 0, -1)], 0)
    s.add_node(m.add_to(s, [mat]))
    s.set_camera((0, 3, 0.01), (0, 0, 0), (0, 1, 0), 40.0, 32, 32)
    return s, s.compile()


@pytest.mark.gpu
def test_upload_refuses_malformed_materials_and_accepts_all_seven_types(ctl, dev):
    gold = (BC.GOLD_ETA, BC.GOLD_K)
    cases = []

    def bad(mat, change, match, drop_ext=False):
        cases.append((mat, change, match, drop_ext))

    def setv(**kw):
        def f(m):
            for k, v in kw.items():
                setattr(m, k, v)
        return f

    for mk in (ctl.dielectric_material, ctl.thindielectric_material):
        bad(mk(1.5), setv(combined_type=R.EDELTA_REFLECTION), "combined_type")
        bad(mk(1.5), setv(eta=0.0), "eta")
        bad(mk(1.5), setv(eta=-1.5), "eta")
        bad(mk(1.5), setv(texture=0), "texture")
    bad(ctl.conductor_material(*gold), setv(combined_type=R.EGLOSSY_REFLECTION), "combined_type")
    bad(ctl.conductor_material(*gold), setv(texture=0), "texture")
    bad(ctl.conductor_material(*gold), setv(), "ctl_material_ext", drop_ext=True)
    bad(ctl.roughconductor_material(1, *gold, 0.3), setv(), "ctl_material_ext", drop_ext=True)
    bad(ctl.roughconductor_material(1, *gold, 0.3), setv(distribution=2), "Beckmann/GGX")
    bad(ctl.roughconductor_material(1, *gold, 0.3), setv(sample_visible=0), "visible-normal")
    bad(ctl.roughconductor_material(1, *gold, 0.3), setv(combined_type=R.EDELTA_REFLECTION), "combined_type")
    bad(ctl.roughconductor_material(1, *gold, 0.3), setv(texture=0), "texture")
    bad(ctl.plastic_material(1.5), setv(), "ctl_material_ext", drop_ext=True)
    bad(ctl.plastic_material(1.5), setv(eta=0.0), "eta")
    bad(ctl.plastic_material(1.5), setv(combined_type=R.EDIFFUSE_REFLECTION), "combined_type")
    bad(ctl.plastic_material(1.5), setv(texture=5), "texture index")
    bad(ctl.diffuse_material(0.5, 0.5, 0.5), setv(bsdf_type=9), "not supported")
    bad(ctl.diffuse_material(0.5, 0.5, 0.5), setv(bsdf_type=2), "not supported")
    t = ctl.Tracer(0)
    try:
        for mat, change, match, drop_ext in cases:
            # compiled well-formed, then damaged in the description (the host compile has checks of its own)
            hs, d = _one_material_scene(ctl, mat, texture=True)
            t.upload_scene(d)
            change(d.materials[0])
            if drop_ext:
                d.materials_ext = None
            with pytest.raises(ctl.CTLError, match=match):
                t.upload_scene(d)
            if "not supported" not in match and "index" not in match:
                assert "material 0" in str(pytest.raises(ctl.CTLError, t.upload_scene, d).value)
        t.upload_scene(BC.host_scene()[1])   # diffuse, roughdielectric and the five new types
        types = {BC.host_scene()[1].materials[i].bsdf_type for i in range(BC.host_scene()[1].n_materials)}
        assert types == {1, 3, 4, 5, 6, 7, 8}
        # a textured plastic is accepted
        s, d = _one_material_scene(ctl, ctl.plastic_material(1.5, texture=0), texture=True)
        t.upload_scene(d)
    finally:
        t.close()


# ---------------------------------------------------------------------------------------------
def mixed_scene(ctl, w=48, h=48):
    """A diffuse floor, an area light, the environment, and one tilted card per new type."""
    s = ctl.HostScene()
    rng = np.random.default_rng(5)
    yy = np.arange(8)[:, None]
    img = ((40 + 20 * yy + rng.integers(0, 30, size=(8, 16))).astype(np.uint32) * 0x010101) | 0xff000000
    s.set_environment(s.add_texture(img.astype(np.uint32), filter=ctl._abi.CTL_TEX_BILINEAR), (1.5, 1.4, 1.3))
    gold = (BC.GOLD_ETA, BC.GOLD_K)
    mats = [ctl.diffuse_material(0.6, 0.6, 0.55), ctl.diffuse_material(0.8, 0.8, 0.8),
            ctl.dielectric_material(1.5), ctl.thindielectric_material(1.5, (0.9, 0.9, 1.0), (0.9, 1.0, 0.9)),
            ctl.conductor_material(*gold, (0.95, 0.9, 0.85)), ctl.roughconductor_material(1, *gold, 0.2),
            ctl.plastic_material(1.5, (0.2, 0.4, 0.7), nonlinear=True)]
    m = Mesh()
    m.quad([(-6, 0, -6), (-6, 0, 6), (6, 0, 6), (6, 0, -6)], 0)
    m.quad([(-0.8, 3.0, -0.8), (0.8, 3.0, -0.8), (0.8, 3.0, 0.8), (-0.8, 3.0, 0.8)], 1)   # light, facing down
    for k in range(5):   # cards leaning back, facing the camera and the sky
        x = -2.6 + 1.3 * k
        m.quad([(x - 0.55, 0.05, -0.3), (x + 0.55, 0.05, -0.3), (x + 0.55, 1.3, 0.5), (x - 0.55, 1.3, 0.5)], 2 + k)
    node = s.add_node(m.add_to(s, mats))
    s.add_area_light(node, 1, (14.0, 14.0, 14.0))
    s.set_camera((0.3, 2.0, -5.5), (0.0, 0.6, 0.0), (0, 1, 0), 50.0, w, h)
    return s, s.compile()


@pytest.mark.gpu
@pytest.mark.parametrize("direct", [1, 0])
@pytest.mark.parametrize("bvh", ["wide", "binary"])
def test_schedules_agree_on_the_mixed_scene(ctl, dev, direct, bvh):
    w, h, passes = 48, 48, 3
    hs, d = mixed_scene(ctl, w, h)
    if bvh == "binary":
        d = binary_bvh(d)
    base = render(ctl, d, ctl.PTParams(direct, 12, 3, 1, 16, 1, 0, 0), passes, w, h, dev)
    assert np.isfinite(base).all() and (base[:, 6] > 0).sum() > 0.9 * w * h
    assert base[:, :3].max() > 0.0
    for flags in (ctl.CTL_PT_MEGAKERNEL, ctl.CTL_PT_WAVEFRONT):
        assert same(base, render(ctl, d, ctl.PTParams(direct, 12, 3, 1, 16, 1, 0, flags), passes, w, h, dev)), flags
    assert same(base, render(ctl, d, ctl.PTParams(direct, 12, 3, 1, 16, 1, 0, 0), passes, w, h, dev, batched=True))
    acc = np.zeros_like(base)
    for r in range(3):
        acc += render(ctl, d, ctl.PTParams(direct, 12, 3, 1, 16, 3, r, 0), passes, w, h, dev)
    assert same(acc, base)


@pytest.mark.gpu
def test_materials_change_the_image(ctl, dev):
    """The five cards are shaded by their own BSDFs: each differs from the same card in diffuse grey."""
    w, h = 48, 48
    hs, d = mixed_scene(ctl, w, h)
    p = ctl.PTParams(1, 12, 3, 1, 16, 1, 0, 0)
    base = render(ctl, d, p, 2, w, h, dev)
    for k in range(2, 7):
        m = ctl._abi.Material.from_buffer_copy(d.materials[k])
        try:
            d.materials[k] = ctl.diffuse_material(0.5, 0.5, 0.5)
            assert not same(base, render(ctl, d, p, 2, w, h, dev)), k
        finally:
            d.materials[k] = m


@pytest.mark.gpu
def test_wpt_and_prim_run_the_mixed_scene(ctl, dev):
    w, h = 48, 48
    hs, d = mixed_scene(ctl, w, h)

    def wpt(direct):
        t = ctl.WavefrontPathTracer(0, direct=direct, max_path_length=8, rr_start_depth=3)
        try:
            t.upload_scene(d)
            fb = torch.zeros((w * h, 7), dtype=torch.float32, device=dev)
            for k in range(2):
                t.do_pass(fb.data_ptr(), 1 + k, new_trace=(k == 0))
            torch.cuda.synchronize()
            return fb.cpu().numpy()
        finally:
            t.close()

    def prim(mode):
        t = ctl.PrimTracer(0, draw_mode=mode)
        try:
            t.upload_scene(d)
            fb = torch.zeros((w * h, 7), dtype=torch.float32, device=dev)
            t.do_pass(fb.data_ptr(), 3)
            torch.cuda.synchronize()
            return fb.cpu().numpy()
        finally:
            t.close()

    for direct in (True, False):
        a, b = wpt(direct), wpt(direct)
        assert same(a, b) and np.isfinite(a).all() and a[:, :3].max() > 0
    for mode in ("first_f", "first_f_direct", "first_Le", "n_shade_colored"):
        a, b = prim(mode), prim(mode)
        assert same(a, b) and np.isfinite(a).all()
    assert prim("first_f_direct")[:, :3].max() > 0
    # the first_non_delta modes need the delta bounce loop, which is not built: refused, not guessed
    with pytest.raises(ctl.CTLError, match="first_non_delta"):
        prim("first_non_delta_f")


# ---------------------------------------------------------------------------------------------
def _env_only(ctl, w, h, cam):
    s = ctl.HostScene()
    uniform_env(s, ctl)
    s.set_camera(*cam, w, h)
    return s, s.compile()


@pytest.mark.gpu
@pytest.mark.parametrize("direct", [1, 0])
def test_invisible_panes(ctl, orc, dev, direct):
    """thindielectric panes with reflectance = transmittance = 1 under a one-colour environment and
    nothing else: every event multiplies the throughput by exactly 1 (sample's weight is the
    reflectance or the transmittance), a delta bounce skips Russian roulette, and the escaped path's
    MIS weight is 1 after a specular bounce, so each sample adds 1 * EvalEnvironment(last ray).

    Bound: the bilinear lookup of a constant c is sum of four terms (1-ds)(1-dt) c, each with at most 4
    roundings (two differences, two products), summed with 3 additions: within 7 * 2^-24 of c; the
    scale product 1 more; the framebuffer's 4 samples are summed with 3 additions: 11 * 2^-24.  The
    render with the panes looks the constant up in other directions than the render without, so the
    two differ by at most 22 * 2^-24 relative.  A lost branch, a wrong weight or roulette on a delta
    bounce shows at 1e-2 or more."""
    w, h, passes = 32, 32, 4
    cam = ((0.0, 0.2, 5.0), (0.0, 0.0, 0.0), (0, 1, 0), 40.0)
    s = ctl.HostScene()
    uniform_env(s, ctl)
    m = Mesh()
    for k, z in enumerate((0.0, 0.7, 1.5, 2.2)):   # overlapping in depth, of different sizes, one tilted
        e = 3.0 - 0.6 * k
        t = 0.4 if k == 2 else 0.0
        m.quad([(-e, -e, z - t), (e, -e, z - t), (e, e, z + t), (-e, e, z + t)], 0)
    s.add_node(m.add_to(s, [ctl.thindielectric_material(1.5, (1.0, 1.0, 1.0), (1.0, 1.0, 1.0))]))
    s.set_camera(*cam, w, h)
    d = s.compile()
    p = ctl.PTParams(direct, 50, 5, 1, 64, 1, 0, 0)
    got = render(ctl, d, p, passes, w, h, dev)
    _, d0 = _env_only(ctl, w, h, cam)
    want, _ = oracle_render(orc, d0, p, passes, w, h)
    assert np.array_equal(got[:, 6], want[:, 6]) and want[:, 6].max() >= passes - 1
    lit = want[:, 6] > 0
    rel = np.abs(got[lit, :3].astype(np.float64) / want[lit, :3].astype(np.float64) - 1.0)
    print(f"invisible panes, direct {direct}: worst {rel.max() / U:.2f} roundings")
    assert rel.max() <= 22 * U
    # the panes are in the way of most primary rays
    t = ctl.Tracer(0)
    try:
        t.upload_scene(d)
        rays = np.zeros((w * h, 8), np.float32)
        orc.oracle_camera_rays(C.byref(d), 0, oracle.ptr(rays))
        dr = torch.from_numpy(rays).to(dev)
        hits = torch.zeros((w * h, 4), dtype=torch.int32, device=dev)
        t.intersect_buffers(w * h, dr.data_ptr(), hits.data_ptr())
        torch.cuda.synchronize()
        assert (hits.cpu().numpy()[:, 2] >= 0).sum() > 0.8 * w * h
    finally:
        t.close()


def _half(h16):
    return np.array([h16], np.uint16).view(np.float16).astype(np.float32)[0]


@pytest.mark.gpu
def test_mirror_wall(ctl, orc, dev):
    """One conductor quad in the plane z = 0 filling the view, facing +z (the axis whose
    spherical-normal code, 0, decodes to (0, 0, 1) exactly: sin 0 and cos 0; the y axis does not,
    its code decodes through cos(fp32 pi / 2) != 0).  max_path_length 2, Direct 0, one pass: a
    pixel's sample is reflectance * fresnelConductorExact(wi.z) * EvalEnvironment(reflected ray),
    wi.z = dot(-d, sys.n) with sys.n = (0, 0, nz).  nz comes out of three normalisations x * (1 / x)
    of vectors along one axis, the first of x = (u + v) + (1 - u - v), the hit's barycentrics; such a
    product is 1 or 1 - 2^-24, never more (1 / x is within 2^-24 relative of exact, so the product
    lies within [1 - 2^-24, 1 + 2^-24] before it is rounded, and the upper tie rounds to 1).  So
    wi.z is -d.z or its neighbour below, and either is accepted.  The environment factor lies in the
    value range of the render without the quad (the constant map, up to the lookup's rounding), and
    the fp32 product may be one ulp off either end of that range (the reflected rays look the
    constant up at other positions than the rays the range was measured on)."""
    w, h = 32, 32
    cam = ((0.3, 0.2, 4.0), (0.0, 0.0, 0.0), (0, 1, 0), 35.0)
    refl = (0.9, 0.75, 0.6)
    s = ctl.HostScene()
    uniform_env(s, ctl)
    m = Mesh()
    m.quad([(-4, -4, 0), (4, -4, 0), (4, 4, 0), (-4, 4, 0)], 0)
    s.add_node(m.add_to(s, [ctl.conductor_material(BC.GOLD_ETA, BC.GOLD_K, refl)]))
    s.set_camera(*cam, w, h)
    d = s.compile()
    # the compiled TriangleData: all six vertex normals carry code 0, dpdu and dpdv are axis vectors
    for t in range(2):
        wds = d.tri_data[t].w
        assert wds[0] == 0 and (wds[1] & 0xffff) == 0
        dpdu = [_half(wds[2] & 0xffff), _half(wds[2] >> 16), _half(wds[3] & 0xffff)]
        dpdv = [_half(wds[3] >> 16), _half(wds[4] & 0xffff), _half(wds[4] >> 16)]
        assert dpdu[1] == 0 and dpdu[2] == 0 and dpdu[0] > 0 and dpdv[0] == 0 and dpdv[2] == 0 and dpdv[1] > 0, (dpdu, dpdv)
    p = ctl.PTParams(0, 2, 5, 1, 64, 1, 0, 0)
    got = render(ctl, d, p, 1, w, h, dev)
    _, d0 = _env_only(ctl, w, h, cam)
    env, _ = oracle_render(orc, d0, p, 1, w, h)
    lo, hi = env[env[:, 6] > 0, :3].min(axis=0), env[:, :3].max(axis=0)
    # the constant map, up to the bilinear lookup's rounding: 8 roundings either way (test_invisible_panes)
    assert (hi.astype(np.float64) / lo.astype(np.float64) - 1.0).max() <= 16 * U * (1 + 1e-3)
    inf = np.float32(np.inf)
    rays = np.zeros((w * h, 8), np.float32)
    orc.oracle_camera_rays(C.byref(d), 0, oracle.ptr(rays))
    lx, ly = jitter_landing(orc, 0, w, h)
    inside = (lx < w) & (ly < h)
    target = ly * w + lx
    count = np.bincount(target[inside], minlength=w * h)
    assert np.array_equal(count.astype(np.float32), got[:, 6])
    checked = 0
    for i in np.nonzero(inside)[0]:
        if count[target[i]] != 1:
            continue
        px = got[target[i], :3]
        ok = False
        for cos in (np.float32(-rays[i, 6]), np.nextafter(np.float32(-rays[i, 6]), np.float32(0))):
            F = R.fresnel_conductor_exact(cos, BC.GOLD_ETA, BC.GOLD_K)
            f = np.array([np.float32(refl[c]) * F[c] for c in range(3)], np.float32)
            ok = ok or ((px >= np.nextafter(f * lo, -inf)).all() and (px <= np.nextafter(f * hi, inf)).all())
        assert ok, (i, px, f * lo, f * hi)
        checked += 1
    assert checked > 0.9 * w * h


@pytest.mark.gpu
@pytest.mark.parametrize("nonlinear", [False, True])
def test_textured_plastic_equals_constant_plastic(ctl, dev, nonlinear):
    """A plastic floor under an area light, NEE on: the image with m_diffuseReflectance an image
    texture of one colour equals the image with the constant reflectance of that colour (the texel
    80 / 255 decodes to the same float the constant is given as)."""
    w, h = 32, 32
    c = np.float32(80) / np.float32(255)

    def scene(textured):
        s = ctl.HostScene()
        # a point-sampled texel is the colour itself (a bilinear lookup of equal texels rounds)
        tex = s.add_texture(np.full((8, 8), 0xff505050, np.uint32), filter=ctl._abi.CTL_TEX_POINT)
        pl = ctl.plastic_material(1.5, (c, c, c), nonlinear=nonlinear, texture=tex if textured else None)
        m = Mesh()
        m.quad([(-3, 0, -3), (-3, 0, 3), (3, 0, 3), (3, 0, -3)], 0)
        m.quad([(-0.5, 2.0, -0.5), (0.5, 2.0, -0.5), (0.5, 2.0, 0.5), (-0.5, 2.0, 0.5)], 1)
        node = s.add_node(m.add_to(s, [pl, ctl.diffuse_material(0.8, 0.8, 0.8)]))
        s.add_area_light(node, 1, (10.0, 10.0, 10.0))
        s.set_camera((0.2, 1.5, -4.0), (0.0, 0.0, 0.0), (0, 1, 0), 50.0, w, h)
        return s, s.compile()

    p = ctl.PTParams(1, 6, 3, 1, 64, 1, 0, 0)
    (s1, d1), (s2, d2) = scene(True), scene(False)
    assert d1.materials[0].texture == 0 and d2.materials[0].texture == 0xFFFFFFFF
    a, b = render(ctl, d1, p, 3, w, h, dev), render(ctl, d2, p, 3, w, h, dev)
    assert same(a, b)
    assert a[:, :3].max() > 0 and np.isfinite(a).all()
    for flags in (ctl.CTL_PT_MEGAKERNEL, ctl.CTL_PT_WAVEFRONT):
        assert same(a, render(ctl, d1, ctl.PTParams(1, 6, 3, 1, 64, 1, 0, flags), 3, w, h, dev))
