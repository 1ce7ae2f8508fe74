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
import materials_scenes as MS
import oracle
from helpers import binary_bvh, oracle_render, tie_rule
from materials_scenes import Mesh, mixed_scene, same


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


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


# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_batch_entry_equals_the_host_entry_bit_for_bit(ctl, dev):
    """ctl_bsdf_eval (HIP) against ctl_host_bsdf_eval on the directed query sets of the four delta
    types (>= 4000 each) and on sample / f / pdf queries of the rough conductors."""
    _, desc = BC.host_scene()
    sets = {t: BC.delta_queries(t) for t in (R.DIELECTRIC, R.THINDIELECTRIC, R.CONDUCTOR, R.PLASTIC)}
    sets[R.ROUGHCONDUCTOR] = BC.roughconductor_queries()
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
def test_wpt_and_prim_run_the_mixed_scene(ctl, orc, dev):
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

    def wpt_oracle(direct):
        fb = np.zeros((w * h, 7), np.float32)
        for k in range(2):
            orc.oracle_wpt_render_pass(C.byref(d), int(direct), 8, 3, k + 1, 1 + k, oracle.ptr(fb), tie_rule(d, orc), 0)
        return fb

    def prim_oracle(mode):
        fb, depth = np.zeros((w * h, 7), np.float32), np.zeros(w * h, np.float32)
        pp = ctl.PrimParams(ctl._abi.PRIM_DRAW_MODES.index(mode), 7, 1.0, 100000.0, 0)
        orc.oracle_prim_pass(C.byref(d), C.byref(pp), 3, oracle.ptr(fb), oracle.ptr(depth), tie_rule(d, orc), 0)
        return fb

    for direct in (True, False):
        a, b = wpt(direct), wpt_oracle(direct)
        assert same(a, b), MS.first_differences(a, b, w)
        assert np.isfinite(a).all() and a[:, :3].max() > 0
    for mode in ("first_f", "first_f_direct", "first_Le", "n_shade_colored"):
        a, b = prim(mode), prim_oracle(mode)
        assert same(a, b), (mode, MS.first_differences(a, b, w))
        assert np.isfinite(a).all()
    assert prim("first_f_direct")[:, :3].max() > 0
    # the first_non_delta modes need the delta bounce loop, which is not built: refused, not guessed
    with pytest.raises(ctl.CTLError, match="first_non_delta"):
        prim("first_non_delta_f")


# ---------------------------------------------------------------------------------------------
# Three renders whose pixels are known in closed form.  The scenes and the checks (with the bounds'
# derivations) are in materials_scenes.py; tests/test_oracle_materials.py applies the same checks to
# the oracle's images.
@pytest.mark.gpu
@pytest.mark.parametrize("direct", [1, 0])
def test_invisible_panes(ctl, orc, dev, direct):
    """thindielectric panes with reflectance = transmittance = 1 under a one-colour environment and
    nothing else: the image equals the environment's within 22 * 2^-24 (MS.check_invisible_panes).  A
    lost branch, a wrong weight or roulette on a delta bounce shows at 1e-2 or more."""
    w, h, passes = 32, 32, 4
    s, d = MS.invisible_panes_scene(ctl, w, h)
    p = ctl.PTParams(direct, 50, 5, 1, 64, 1, 0, 0)
    got = render(ctl, d, p, passes, w, h, dev)
    s0, d0 = MS.env_only(ctl, w, h, MS.PANES_CAM)
    want, _ = oracle_render(orc, d0, p, passes, w, h)
    MS.check_invisible_panes(got, want, passes, f"direct {direct}")
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


@pytest.mark.gpu
def test_mirror_wall(ctl, orc, dev):
    """One conductor quad in the plane z = 0 filling the view, max_path_length 2, Direct 0, one pass: a
    pixel's sample is reflectance * fresnelConductorExact(wi.z) * EvalEnvironment(reflected ray),
    bracketed by nextafter as MS.check_mirror_wall derives."""
    w, h = 32, 32
    s, d = MS.mirror_wall_scene(ctl, w, h)
    p = ctl.PTParams(0, 2, 5, 1, 64, 1, 0, 0)
    got = render(ctl, d, p, 1, w, h, dev)
    s0, d0 = MS.env_only(ctl, w, h, MS.MIRROR_CAM)
    env, _ = oracle_render(orc, d0, p, 1, w, h)
    MS.check_mirror_wall(orc, got, env, d, w, h)


@pytest.mark.gpu
@pytest.mark.parametrize("nonlinear", [False, True])
def test_textured_plastic_equals_constant_plastic(ctl, dev, nonlinear):
    """A plastic floor under an area light, NEE on: the image with m_diffuseReflectance an image
    texture of one colour equals the image with the constant reflectance of that colour, bit for bit."""
    w, h = 32, 32
    p = ctl.PTParams(1, 6, 3, 1, 64, 1, 0, 0)
    (s1, d1), (s2, d2) = MS.textured_plastic_scene(ctl, nonlinear, True), MS.textured_plastic_scene(ctl, nonlinear, False)
    a, b = render(ctl, d1, p, 3, w, h, dev), render(ctl, d2, p, 3, w, h, dev)
    MS.check_textured_plastic(a, b)
    for flags in (ctl.CTL_PT_MEGAKERNEL, ctl.CTL_PT_WAVEFRONT):
        assert same(a, render(ctl, d1, ctl.PTParams(1, 6, 3, 1, 64, 1, 0, flags), 3, w, h, dev))
