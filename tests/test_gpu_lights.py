"""Point, spot and distant lights on the GPU: the batch light entry against its host twin bit for
bit, renders of a lit floor whose pixels are known in closed form (PrimTracer, PathTracer,
WavefrontPathTracer), shadows, the schedules of the PathTracer against each other, and a light moved
by ctl_scene_update.  Images are 64 x 64; no test hands the oracle a scene with one of the new kinds."""
import numpy as np
import pytest
import torch

import light_cases as LC
from helpers import binary_bvh
from materials_scenes import first_differences, same
from test_lights_host import BAND, COS_EXCLUDE

W = H = 64
REL = 1e-4      # the renders' relative tolerance (derived at check_render)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _fb(dev):
    return torch.zeros((W * H, 7), dtype=torch.float32, device=dev)


def device_light_eval(ctl, t, q, dev):
    dq = torch.from_numpy(np.frombuffer(q.tobytes(), np.uint8).copy()).to(dev)
    dr = torch.zeros(len(q) * 64, dtype=torch.uint8, device=dev)
    t.light_eval(len(q), dq.data_ptr(), dr.data_ptr())
    torch.cuda.synchronize()
    return np.frombuffer(dr.cpu().numpy().tobytes(), dtype=ctl.LIGHT_RESULT_DTYPE)


def same_records(a, b):
    """Indices where two result arrays differ in any bit (NaN payloads included)."""
    ua = np.frombuffer(a.tobytes(), np.uint32).reshape(len(a), -1)
    ub = np.frombuffer(b.tobytes(), np.uint32).reshape(len(b), -1)
    return np.nonzero((ua != ub).any(axis=1))[0]


# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_evaluator_equals_the_host_evaluator_bit_for_bit(ctl, dev):
    """ctl_light_eval (HIP) against ctl_host_light_eval on every query of the host tests (random
    sets and edge queries, ref == pos with its NaNs included) and on 1024 queries each against the
    area light and the environment of the mixed scene."""
    rng = np.random.default_rng(17)
    s, _ = LC.mixed_host_scene(ctl)
    mixed = s.compile()
    refs = LC.f32(rng.uniform(-3, 3, size=(1024, 3)) * [1, 0.4, 1] + [0, 0.5, 0])
    area_env = [(f"mixed light {k}", LC.queries(ctl, k, refs, sample=rng.random((1024, 2)))) for k in range(5)]
    groups = [(LC.eval_scene(ctl)[1], [(n, q) for n, q, _ in LC.random_sets(ctl)]),
              (LC.edge_scene(ctl)[1], list(LC.edge_sets(ctl).items())),
              (mixed, area_env)]
    t = ctl.Tracer(0)
    try:
        for desc, sets in groups:
            t.upload_scene(desc)
            for name, q in sets:
                got, want = device_light_eval(ctl, t, q, dev), ctl.host_light_eval(desc, q)
                bad = same_records(got, want)
                assert bad.size == 0, (name, len(bad), q[bad[0]], got[bad[0]], want[bad[0]])
        # the mixed set reached light on both old kinds
        for k in (0, 1):
            want = ctl.host_light_eval(mixed, area_env[k][1])
            assert (want["value"].max(axis=1) > 0).sum() > 100, k
            assert set(want["measure"][want["pdf"] > 0]) == {1}
    finally:
        t.close()


@pytest.mark.gpu
def test_upload_refuses_malformed_delta_lights(ctl, dev):
    s, lights = LC.mixed_host_scene(ctl)
    d = s.compile()
    A = ctl._abi
    t = ctl.Tracer(0)

    def slot(i):
        return A.LightParams.from_buffer(d.light_tris[d.lights[i].tri_first])

    def damaged(change, restore, match):
        change()
        try:
            with pytest.raises(ctl.CTLError, match=match):
                t.upload_scene(d)
        finally:
            restore()

    try:
        t.upload_scene(d)
        sp, ds = slot(3), slot(4)
        first = d.lights[2].tri_first
        damaged(lambda: setattr(d.lights[2], "tri_first", d.n_light_tris), lambda: setattr(d.lights[2], "tri_first", first), "slot")
        damaged(lambda: setattr(d.lights[2], "kind", 5), lambda: setattr(d.lights[2], "kind", 2), "kind")
        x = sp.pos[0]
        damaged(lambda: sp.pos.__setitem__(0, float("nan")), lambda: sp.pos.__setitem__(0, x), "non-finite")
        n = list(ds.n)
        damaged(lambda: ds.n.__setitem__(slice(0, 3), [2 * v for v in n]), lambda: ds.n.__setitem__(slice(0, 3), n), "unit")
        cb = sp.cos_beam_width
        damaged(lambda: setattr(sp, "cos_beam_width", sp.cos_cutoff_angle - 0.01), lambda: setattr(sp, "cos_beam_width", cb),
                "cos_cutoff_angle")
        itw = sp.inv_transition_width
        damaged(lambda: setattr(sp, "inv_transition_width", float("-inf")), lambda: setattr(sp, "inv_transition_width", itw),
                "non-finite")
        sp.inv_transition_width = float("inf")        # +inf is the one infinity upload accepts
        t.upload_scene(d)
        sp.inv_transition_width = itw
        # a refused update leaves the uploaded scene whole
        fb0, fb1 = _fb(dev), _fb(dev)
        pt = ctl.PathTracer(0, max_path_length=4)
        try:
            pt.upload_scene(d)
            pt.do_pass(fb0.data_ptr(), 0)
            sp.pos[0] = float("nan")
            with pytest.raises(ctl.CTLError, match="non-finite"):
                pt.update_scene(d, A.CTL_DIRTY_LIGHTS)
            sp.pos[0] = x
            pt.do_pass(fb1.data_ptr(), 0)
            torch.cuda.synchronize()
            assert same(fb0.cpu().numpy(), fb1.cpu().numpy())
        finally:
            pt.close()
    finally:
        t.close()


# ---------------------------------------------------------------------------------------------
# Analytic renders.  A ray from the camera through sample position (sx, sy) meets the floor at P; the
# one light sample gives rho / pi * cos(theta) * E(P) (times the integrator's own weight), with E the
# float64 irradiance term of light_ref.py.
#
# Tolerance 1e-4 relative: a pixel is reached in under 100 fp32 roundings (camera ray, Woop hit, P,
# the light sample, the frame at the hit, the BSDF value and the products), about 6e-6 if all err the
# same way; the steps that amplify are cos(theta) and the camera ray's cosine at up to 60 degrees,
# a conditioning of at most 4.  A dropped factor (1 / pi, cos, 1 / d^2, the falloff) moves the value
# by far more.  Inside the spot's band the falloff's absolute tolerance of test_lights_host (BAND x
# inv_transition_width, scaled by the pixel's other factors) is added.
def expected_samples(kind, d, sx, sy, weight=None, L=None):
    """Per sample: float64 rgb value of the direct term, and whether to leave the sample out (the spot's
    cosTheta within COS_EXCLUDE of a threshold), and the absolute tolerance."""
    o, dirs = LC.pixel_corner_rays(d, sx, sy)
    P = LC.floor_points(o, dirs)
    E, cos_t, r = LC.irradiance(kind, P, L)
    assert np.all(cos_t > 0.5) and np.all(-dirs[:, 2] > 0.5)          # within 60 degrees of the normal
    f = np.asarray(LC.RHO, np.float64)[None, :] / np.pi * cos_t[:, None]
    if weight is not None:
        f = f * weight(cos_t)[:, None]
    val = f * E
    tol = REL * val
    skip = np.zeros(len(sx), bool)
    regions = None
    if kind == "spot":
        sp = LC.ANALYTIC["spot"] if L is None else L
        cc, cb = np.cos(np.radians(np.float64(sp["cutoff"]))), np.cos(np.radians(np.float64(sp["beam"])))
        ct = r["cos_theta"]
        skip = (np.abs(ct - cc) <= COS_EXCLUDE) | (np.abs(ct - cb) <= COS_EXCLUDE)
        band = (ct > cc) & (ct < cb)
        itw = 1.0 / (np.radians(np.float64(sp["cutoff"])) - np.radians(np.float64(sp["beam"])))
        tol = tol + np.where(band[:, None], BAND * itw * f * r["unattenuated"], 0.0)
        regions = (ct >= cb, band, ct <= cc)
    return val, tol, skip, regions


def check_render(name, got, val, tol, skip, pixel, extra=0.0, max_skipped=0.02):
    """got: framebuffer rows; sample k (value val[k]) landed on pixel[k] (-1: outside the image)."""
    n = W * H
    want, wtol, cnt = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
    bad = np.zeros(n, bool)
    inside = pixel >= 0
    np.add.at(want, pixel[inside], val[inside])
    np.add.at(wtol, pixel[inside], tol[inside])
    np.add.at(cnt, pixel[inside], 1)
    bad[pixel[inside & skip]] = True
    assert bad.sum() <= max_skipped * n, (name, int(bad.sum()))
    ok = ~bad
    assert np.array_equal(got[ok, 6], cnt[ok].astype(np.float32)), name
    want = want + extra * cnt[:, None]
    err = np.abs(got[ok, :3].astype(np.float64) - want[ok])
    lim = wtol[ok] + REL * extra * cnt[ok, None]
    rel = (err / np.maximum(want[ok], 1e-300)).max()
    print(f"{name}: worst error / tolerance {(err / np.maximum(lim, 1e-300)).max():.4f}, worst relative error {rel:.3e}, "
          f"{int(bad.sum())} pixels left out")
    assert np.all(err <= lim), (name, float((err / np.maximum(lim, 1e-300)).max()))
    assert want[ok].max() > 0.01


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["point", "spot", "distant"])
def test_prim_tracer_renders_the_analytic_floor(ctl, dev, kind):
    """ctl_prim_pass, first_f_direct: one un-jittered ray per pixel through the pixel's corner; the
    pixel is rho / pi * cos(theta) * E + rho / (2 pi)."""
    s, d = LC.analytic_scene(ctl, kind)
    assert LC.floor_normals_exact(ctl, d)
    ys, xs = np.mgrid[0:H, 0:W]
    sx, sy = xs.ravel().astype(np.float64), ys.ravel().astype(np.float64)
    val, tol, skip, regions = expected_samples(kind, d, sx, sy)
    if regions is not None:
        for r in regions:     # plateau, band, dark: each at least 10 % of the pixels
            assert r.sum() >= 0.1 * W * H, [int(x.sum()) for x in regions]
    t = ctl.PrimTracer(0, draw_mode="first_f_direct")
    try:
        t.upload_scene(d)
        fb = _fb(dev)
        t.do_pass(fb.data_ptr(), 0)
        torch.cuda.synchronize()
        got = fb.cpu().numpy()
    finally:
        t.close()
    # f_avg * 0.5 = rho / (2 pi) on every channel: the tolerance takes the channels' largest
    base = np.asarray(LC.RHO, np.float64) / (2 * np.pi)
    check_render(f"prim {kind}", got, val + base[None, :], tol + REL * base[None, :], skip, np.arange(W * H))


def pass_rays(ctl, pt, d, dev, pass_index):
    """The pass's camera rays (ctl_camera_rays) and, per ray, its sample position recovered by
    projecting the direction back through the camera in float64, and the pixel it lands on (-1:
    outside).  near: the position is within 1e-4 pixel of a pixel border, so the pixel the device's
    fp32 position falls in cannot be told (the recovery is good to about 64 * 1e-7 pixels)."""
    pt.generate_samples(pass_index)
    n = pt.camera_rays()
    assert n == W * H
    rays = torch.zeros((n, 8), dtype=torch.float32, device=dev)
    pt.camera_rays(rays.data_ptr(), n)
    torch.cuda.synchronize()
    sx, sy = LC.back_project(d, rays.cpu().numpy()[:, 4:7].astype(np.float64))
    near = (np.abs(sx - np.round(sx)) < 1e-4) | (np.abs(sy - np.round(sy)) < 1e-4)
    px, py = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    pixel = np.where((px >= 0) & (px < W) & (py >= 0) & (py < H), py * W + px, -1)
    return sx, sy, pixel, near


def render_pt(ctl, d, dev, params, pass_index=0, want_rays=True):
    pt = ctl.PathTracer(0)
    try:
        pt.upload_scene(d)
        pt.params = params
        geo = pass_rays(ctl, pt, d, dev, pass_index) if want_rays else None
        fb = _fb(dev)
        pt.do_pass(fb.data_ptr(), pass_index)
        torch.cuda.synchronize()
        return fb.cpu().numpy(), geo
    finally:
        pt.close()


def with_neighbours(pixel, near):
    """Pixels a sample near a pixel border may have landed on: its own and the eight around it."""
    out = []
    for p in pixel[near & (pixel >= 0)]:
        x, y = int(p) % W, int(p) // W
        out += [yy * W + xx for yy in (y - 1, y, y + 1) for xx in (x - 1, x, x + 1) if 0 <= xx < W and 0 <= yy < H]
    return np.array(sorted(set(out)), np.int64)


def check_jittered(name, got, kind, d, geo, weight=None, L=None):
    sx, sy, pixel, near = geo
    val, tol, skip, _ = expected_samples(kind, d, sx, sy, weight, L)
    amb = with_neighbours(pixel, near)
    skip = skip.copy()
    skip |= np.isin(pixel, amb)
    check_render(name, got, val, tol, skip, pixel)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["point", "spot", "distant"])
def test_path_tracer_renders_the_analytic_floor(ctl, dev, kind):
    """PathTracer, Direct = 1, MaxPathLength = 1: a sample is the one light sample at the first hit,
    rho / pi * cos(theta) * E (a discrete sample takes no heuristic weight)."""
    s, d = LC.analytic_scene(ctl, kind)
    got, geo = render_pt(ctl, d, dev, ctl.PTParams(1, 1, 5, 1, 64, 1, 0, 0))
    check_jittered(f"pt {kind}", got, kind, d, geo)


def render_wpt(ctl, d, dev, pass_index=0):
    # MaxPathLength 2: iteration 0 shades the first hit and draws its one light sample (wpt.hip: the
    # sample is drawn when depth + 1 != MaxPathLength), iteration 1 collects it and ends the path
    t = ctl.WavefrontPathTracer(0, direct=True, max_path_length=2, rr_start_depth=5)
    try:
        t.upload_scene(d)
        fb = _fb(dev)
        t.do_pass(fb.data_ptr(), pass_index, new_trace=True)
        torch.cuda.synchronize()
        return fb.cpu().numpy()
    finally:
        t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["point", "spot", "distant"])
def test_wavefront_path_tracer_renders_the_analytic_floor(ctl, dev, kind):
    """The WavefrontPathTracer weights a discrete sample too (WavefrontPathTracer.cu:128-129):
    q^2 / (q^2 + (cos(theta) / pi)^2) with q the light's pick probability, here 1.  Its camera sample is
    the PathTracer's (same sampler, same first draw), and its sample lands on the pixel it started from."""
    s, d = LC.analytic_scene(ctl, kind)
    pt = ctl.PathTracer(0)
    try:
        pt.upload_scene(d)
        pt.params = ctl.PTParams(1, 1, 5, 1, 64, 1, 0, 0)
        geo = pass_rays(ctl, pt, d, dev, 0)
    finally:
        pt.close()
    got = render_wpt(ctl, d, dev)
    check_jittered(f"wpt {kind}", got, kind, d, geo, weight=lambda c: 1.0 / (1.0 + (c / np.pi) ** 2))


@pytest.mark.gpu
def test_two_half_lights_render_the_single_light(ctl, dev):
    """Two co-located point lights of half the intensity: each sample picks one with probability 1/2
    and divides by it, so every sample has the single light's value (pick probability and CDF).  The
    WavefrontPathTracer's weight then carries q = 1/2."""
    s1, d1 = LC.analytic_scene(ctl, "point")
    s2, d2 = LC.analytic_scene(ctl, "point", copies=2)
    assert d2.n_lights == 2 and d2.light_cdf[0] == 0.5 and d2.light_cdf[1] == 1.0
    p = ctl.PTParams(1, 1, 5, 1, 64, 1, 0, 0)
    got, geo = render_pt(ctl, d2, dev, p)
    check_jittered("pt two half lights", got, "point", d2, geo)
    one, _ = render_pt(ctl, d1, dev, p, want_rays=False)
    ok = one[:, 6] == 1
    assert np.all(np.abs(got[ok, :3] - one[ok, :3]) <= REL * one[ok, :3])
    check_jittered("wpt two half lights", render_wpt(ctl, d2, dev), "point", d2, geo,
                   weight=lambda c: 0.25 / (0.25 + (c / np.pi) ** 2))


# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("any_hit", [0, 1])
@pytest.mark.parametrize("kind", ["point", "distant"])
def test_shadows(ctl, dev, kind, any_hit):
    """An occluder quad between the light and the floor (outside the camera's view).  Samples whose
    float64 shadow ray passes the quad's interior by more than 1 % of its edge are exactly 0, samples
    that miss it by that margin equal the render without the quad bit for bit; the band between is left
    out (at most 10 % of the image); umbra and lit region each cover at least 20 %."""
    L = LC.SHADOW[kind]
    s0, d0 = LC.analytic_scene(ctl, kind, L=L)
    s1, d1 = LC.analytic_scene(ctl, kind, L=L, occluder=True)
    p = ctl.PTParams(1, 1, 5, any_hit, 64, 1, 0, 0)
    lit_fb, _ = render_pt(ctl, d0, dev, p, want_rays=False)
    got, (sx, sy, pixel, near) = render_pt(ctl, d1, dev, p)
    o, dirs = LC.pixel_corner_rays(d1, sx, sy)
    cls = LC.occluded(kind, LC.floor_points(o, dirs), 0.01)
    n = W * H
    amb = np.zeros(n, bool)
    amb[with_neighbours(pixel, near)] = True
    inside = pixel >= 0
    lo, hi = np.full(n, 2), np.full(n, -2)
    np.minimum.at(lo, pixel[inside], cls[inside])
    np.maximum.at(hi, pixel[inside], cls[inside])
    umbra, lit = (lo == 1) & (hi == 1) & ~amb, (lo == -1) & (hi == -1) & ~amb
    rest = ~(umbra | lit) & (got[:, 6] > 0)
    print(f"shadows {kind} any_hit {any_hit}: umbra {umbra.sum()}, lit {lit.sum()}, left out {rest.sum()}")
    assert umbra.sum() >= 0.2 * n and lit.sum() >= 0.2 * n and rest.sum() <= 0.1 * n
    assert not got[umbra, :3].any() and np.all(got[umbra, 6] >= 1)
    assert same(got[lit], lit_fb[lit]) and lit_fb[lit, :3].min() > 0


# ---------------------------------------------------------------------------------------------
def _render_schedule(ctl, d, dev, flags=0, ranks=1, rank=0, blocks=False, passes=3):
    pt = ctl.PathTracer(0)
    try:
        pt.upload_scene(d)
        pt.params = ctl.PTParams(1, 8, 3, 1, 16, ranks, rank, flags)
        fb = _fb(dev)
        for p in range(passes):
            if blocks:
                pt.generate_samples(p)
                pt.render_pass_blocks(fb.data_ptr(), np.arange((W // 16) * (H // 16), dtype=np.uint32))
            else:
                pt.do_pass(fb.data_ptr(), p)
        torch.cuda.synchronize()
        return fb.cpu().numpy(), pt.rays_traced()
    finally:
        pt.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bvh", ["wide", "binary"])
def test_schedules_agree_on_the_mixed_scene(ctl, dev, bvh):
    """All five kinds of light on a two-instance scene with a textured diffuse and a rough conductor
    material, 3 passes, MaxPathLength 8: megakernel, wavefront, render-ahead, the sum of three shards
    and a block-list pass over all blocks equal the persistent schedule bit for bit, rays included.
    16-pixel tiles, so that the three shards and the block list each hold several tiles."""
    s, _ = LC.mixed_host_scene(ctl, instances=2)
    d = s.compile()
    assert d.n_nodes == 2 and d.n_lights == 5
    if bvh == "binary":
        d = binary_bvh(d)
    base, rays = _render_schedule(ctl, d, dev)
    assert np.isfinite(base).all() and (base[:, 6] > 0).sum() > 0.9 * W * H and base[:, :3].max() > 0
    for name, flags in (("megakernel", ctl.CTL_PT_MEGAKERNEL), ("wavefront", ctl.CTL_PT_WAVEFRONT),
                        ("render-ahead", ctl.CTL_PT_RENDER_AHEAD)):
        got, r = _render_schedule(ctl, d, dev, flags)
        assert same(base, got), (name, first_differences(got, base, W))
        assert r == rays, name
    acc, total = np.zeros_like(base), 0
    for rank in range(3):
        got, r = _render_schedule(ctl, d, dev, ranks=3, rank=rank)
        acc += got
        total += r
    assert same(acc, base) and total == rays
    got, r = _render_schedule(ctl, d, dev, blocks=True)
    assert same(base, got), first_differences(got, base, W)
    assert r == rays
    # the delta lights reach the image: the same scene without them differs
    s0, _ = LC.mixed_host_scene(ctl, instances=2, delta=False)
    d0 = s0.compile()
    other, _ = _render_schedule(ctl, binary_bvh(d0) if bvh == "binary" else d0, dev)
    assert not same(base, other)


@pytest.mark.gpu
def test_moving_a_light_is_a_scene_update(ctl, dev):
    """The point light moved with ctl_scene_update(CTL_DIRTY_LIGHTS) between two passes: the second
    pass equals the second pass of a context that uploaded the moved scene from the start."""
    moved = dict(pos=LC.f32([1.0, 1.25, -2.0]), I=LC.f32([2.0, 4.5, 3.0]))
    s0, _ = LC.mixed_host_scene(ctl)
    s1, _ = LC.mixed_host_scene(ctl, point=moved)
    d0, d1 = s0.compile(), s1.compile()
    p = ctl.PTParams(1, 6, 3, 1, 64, 1, 0, 0)

    def two_passes(first, second):
        pt = ctl.PathTracer(0)
        try:
            pt.upload_scene(first)
            pt.params = p
            a, b = _fb(dev), _fb(dev)
            pt.do_pass(a.data_ptr(), 0)
            if second is not None:
                pt.update_scene(second, ctl._abi.CTL_DIRTY_LIGHTS)
            pt.do_pass(b.data_ptr(), 1)
            torch.cuda.synchronize()
            return a.cpu().numpy(), b.cpu().numpy()
        finally:
            pt.close()

    a0, b_updated = two_passes(d0, d1)
    a1, b_fresh = two_passes(d1, None)
    _, b_unmoved = two_passes(d0, None)
    assert same(b_updated, b_fresh), first_differences(b_updated, b_fresh, W)
    assert not same(a0, a1) and not same(b_updated, b_unmoved)
