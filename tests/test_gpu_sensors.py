"""Thin-lens, orthographic, telecentric and spherical sensors on the GPU: the batch sensor entry against its
host twin bit for bit, ctl_camera_rays against the host evaluator on the pass's own samples, a one-quad render
replayed in float64 in the three integrators, the PathTracer's schedules against each other, the perspective
sensor untouched, and the sensor changed by ctl_scene_update.  Images are 48 x 32 (one partial 64-pixel tile,
aspect != 1) and 80 x 48 (a second tile column); no test hands the oracle a scene with another sensor."""
import ctypes as C

import numpy as np
import pytest
import torch

import sensor_cases as SC
from helpers import binary_bvh
from materials_scenes import first_differences, same
from test_sensors_host import BAD_FIELDS, bad_record

W, H = SC.W, SC.H


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _fb(dev, w=W, h=H):
    return torch.zeros((w * h, 7), dtype=torch.float32, device=dev)


def device_sensor_eval(ctl, t, q, dev):
    dq = torch.from_numpy(np.frombuffer(q.tobytes(), np.uint8).copy()).to(dev)
    dr = torch.zeros(len(q) * ctl.SENSOR_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    t.sensor_eval(len(q), dq.data_ptr(), dr.data_ptr())
    torch.cuda.synchronize()
    return np.frombuffer(dr.cpu().numpy().tobytes(), dtype=ctl.SENSOR_RESULT_DTYPE)


# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_evaluator_equals_the_host_evaluator_bit_for_bit(ctl, dev):
    """ctl_sensor_eval (HIP) against ctl_host_sensor_eval on the query sets of the host tests, all five types,
    sampleRay and sampleRayDifferential; and a description without a record."""
    t = ctl.Tracer(0)
    try:
        for kind in SC.KINDS + (None,):
            _, d = SC.quad_scene(ctl, kind or "perspective", sensor=kind is not None)
            t.upload_scene(d)
            for differential in (False, True):
                for what, q in (("random", SC.random_queries(ctl, differential)), ("edges", SC.edge_queries(ctl, differential))):
                    got, want = device_sensor_eval(ctl, t, q, dev), ctl.host_sensor_eval(d, q)
                    bad = np.nonzero(np.frombuffer(got.tobytes(), np.uint32).reshape(len(q), -1)
                                     != np.frombuffer(want.tobytes(), np.uint32).reshape(len(q), -1))[0]
                    assert bad.size == 0, (kind, differential, what, len(bad), q[bad[0]], got[bad[0]], want[bad[0]])
    finally:
        t.close()


# ---------------------------------------------------------------------------------------------
def device_draws(ctl, pt, draws=2, nseq=4096):
    """Rows 0 .. draws - 1 of the 2-D sampler table the device holds (CTL_ARRAY_SAMPLES_2D)"""
    return np.stack([pt.read_array(ctl._abi.CTL_ARRAY_SAMPLES_2D, k * nseq, nseq, np.float32, 2) for k in range(draws)])


def camera_rays(pt, dev):
    n = pt.camera_rays()
    rays = torch.zeros((n, 8), dtype=torch.float32, device=dev)
    assert pt.camera_rays(rays.data_ptr(), n) == n
    torch.cuda.synchronize()
    return rays.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", SC.NEW_KINDS)
def test_camera_rays_equal_the_host_evaluator(ctl, dev, kind):
    """ctl_camera_rays under each new sensor: per work item (work_pixel's order, restated in sensor_cases.py) the ray
    of sampleRayDifferential for the pixel sample (px, py) + 2-D draw 0 and the aperture sample 2-D draw 1, bit for
    bit; work items outside the image have an empty interval."""
    _, d = SC.quad_scene(ctl, kind)
    pt = ctl.PathTracer(0)
    try:
        pt.upload_scene(d)
        pt.generate_samples(3)
        rays = camera_rays(pt, dev)
        draws = device_draws(ctl, pt)
    finally:
        pt.close()
    assert np.array_equal(draws, SC.host_draws(ctl, 3))
    px, py, inside = SC.work_order(W, H)
    assert len(rays) == len(px) == 64 * 64 and inside.sum() == W * H
    assert np.all(rays[~inside, 7] == 0)
    idx = (py * W + px)[inside]
    pX = np.stack([px, py], 1)[inside].astype(np.float32) + SC.draw2(draws[0], idx)
    want = ctl.host_sensor_eval(d, SC.queries(ctl, pX, SC.draw2(draws[1], idx), True))
    got = rays[inside]
    assert np.array_equal(got[:, 0:3].view(np.uint32), want["o"].view(np.uint32))
    assert np.array_equal(got[:, 4:7].view(np.uint32), want["d"].view(np.uint32))
    assert np.all(got[:, 3] == np.float32(d.ray_eps)) and np.all(got[:, 7] == np.finfo(np.float32).max)
    if kind != "orthographic":
        assert len(np.unique(got[:, 4:7], axis=0)) > W * H // 2          # the sensor is not the pinhole's one direction set
    if kind in ("thinlens", "telecentric"):
        assert len(np.unique(got[:, 0:3], axis=0)) > W * H // 2          # the lens is sampled


# ---------------------------------------------------------------------------------------------
def check_replay(name, got, rp):
    """Every usable pixel holds exactly the samples the replay says landed on it: QUAD_L per path that sees the
    quad, exactly 0 per path that misses, weight 1 each."""
    rgb, weight, usable = SC.expected_image(rp)
    n = W * H
    ok = ~rp["skip"]
    print(f"{name}: hit {int((rp['hit'] & ok).sum())}, miss {int((~rp['hit'] & ok).sum())}, left out {int(rp['skip'].sum())}, "
          f"pixels not usable {int((~usable).sum())}")
    assert rp["skip"].sum() <= 0.02 * n and (~usable).sum() <= 0.02 * n
    assert (rp["hit"] & ok).sum() >= n // 8 and (~rp["hit"] & ok).sum() >= n // 8
    bad = np.nonzero(usable & ((got[:, :3] != rgb).any(axis=1) | (got[:, 6] != weight)))[0]
    assert bad.size == 0, (name, f"{bad.size} pixels differ; first: " + "; ".join(
        f"({int(i) % W}, {int(i) // W}) got {got[i].tolist()} want {rgb[i].tolist()} weight {weight[i]}" for i in bad[:3]))


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", ["persistent", "megakernel", "wavefront"])
@pytest.mark.parametrize("kind", SC.NEW_KINDS)
def test_path_tracer_renders_the_replayed_quad(ctl, dev, kind, schedule):
    """MaxPathLength 1: a pixel is the emission its path's primary ray finds."""
    _, d = SC.quad_scene(ctl, kind)
    pt = ctl.PathTracer(0, max_path_length=1, schedule=schedule)
    try:
        pt.upload_scene(d)
        fb = _fb(dev)
        pt.do_pass(fb.data_ptr(), 0)
        torch.cuda.synchronize()
        draws = device_draws(ctl, pt)
    finally:
        pt.close()
    check_replay(f"{kind} PathTracer {schedule}", fb.cpu().numpy(), SC.replay(ctl, d, "pt", draws))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", SC.NEW_KINDS)
def test_wavefront_path_tracer_renders_the_replayed_quad(ctl, dev, kind):
    """The WavefrontPathTracer calls sampleRay (the replay asks the evaluator for it).  In this scene the two
    functions' rays see the same image; test_the_orthographic_origin_decides_the_image tells them apart."""
    _, d = SC.quad_scene(ctl, kind)
    t = ctl.WavefrontPathTracer(0, max_path_length=1)
    try:
        t.upload_scene(d)
        fb = _fb(dev)
        t.do_pass(fb.data_ptr(), 0, new_trace=True)
        torch.cuda.synchronize()
        draws = device_draws(ctl, t)
    finally:
        t.close()
    check_replay(f"{kind} WavefrontPathTracer", fb.cpu().numpy(), SC.replay(ctl, d, "wpt", draws))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", SC.NEW_KINDS)
def test_prim_tracer_renders_the_replayed_quad(ctl, dev, kind):
    """first_Le: the emission at the first hit.  The pixel sample is the unjittered pixel, the aperture sample the
    PrimTracer's own first 2-D draw."""
    _, d = SC.quad_scene(ctl, kind)
    t = ctl.PrimTracer(0, draw_mode="first_Le")
    try:
        t.upload_scene(d)
        fb = _fb(dev)
        t.do_pass(fb.data_ptr(), 0)
        torch.cuda.synchronize()
        draws = device_draws(ctl, t)
    finally:
        t.close()
    check_replay(f"{kind} PrimTracer", fb.cpu().numpy(), SC.replay(ctl, d, "prim", draws))


@pytest.mark.gpu
def test_the_orthographic_origin_decides_the_image(ctl, dev):
    """The near-quad scene (sensor_cases.py): the quad stands between the plane z = 0 of camera space, where
    Sensor::sampleRay starts, and nearP at z = near, where sampleRayDifferential starts.  The WavefrontPathTracer,
    which calls sampleRay, sees the quad where the sampleRay replay does; the PathTracer (every schedule) and the
    PrimTracer, which call sampleRayDifferential, start behind it and render exactly 0 everywhere.  A camera stage
    that called the other function would give the other image."""
    _, d = SC.near_quad_scene(ctl)
    n = W * H
    t = ctl.WavefrontPathTracer(0, max_path_length=1)
    try:
        t.upload_scene(d)
        fb = _fb(dev)
        t.do_pass(fb.data_ptr(), 0, new_trace=True)
        torch.cuda.synchronize()
        draws = device_draws(ctl, t)
    finally:
        t.close()
    got = fb.cpu().numpy()
    check_replay("near quad, WavefrontPathTracer", got, SC.replay(ctl, d, "wpt", draws, quad_z=SC.NEAR_QUAD_Z))
    assert (got[:, :3] != 0).any(axis=1).sum() >= n // 8
    for schedule in ("persistent", "megakernel", "wavefront"):
        pt = ctl.PathTracer(0, max_path_length=1, schedule=schedule)
        try:
            pt.upload_scene(d)
            fb = _fb(dev)
            pt.do_pass(fb.data_ptr(), 0)
            torch.cuda.synchronize()
        finally:
            pt.close()
        got = fb.cpu().numpy()
        assert not got[:, :3].any() and got[:, 6].sum() > 0.9 * n, schedule
    p = ctl.PrimTracer(0, draw_mode="first_Le")
    try:
        p.upload_scene(d)
        fb = _fb(dev)
        p.do_pass(fb.data_ptr(), 0)
        torch.cuda.synchronize()
    finally:
        p.close()
    got = fb.cpu().numpy()
    assert not got[:, :3].any() and np.all(got[:, 6] == 1)


# ---------------------------------------------------------------------------------------------
SW, SH = 80, 48


def _schedule(ctl, d, dev, flags=0, ranks=1, rank=0, mode="do_pass", passes=3):
    pt = ctl.PathTracer(0)
    try:
        pt.upload_scene(d)
        pt.params = ctl.PTParams(1, 8, 3, 1, 64, ranks, rank, flags)
        fb = _fb(dev, SW, SH)
        if mode == "render_passes":
            pt.render_passes(fb.data_ptr(), 0, passes)
        else:
            for p in range(passes):
                if mode == "blocks":      # every 64-pixel block of the image, through ctl_render_pass_blocks
                    pt.generate_samples(p)
                    pt.render_pass_blocks(fb.data_ptr(), np.arange(-(-SW // 64) * -(-SH // 64), dtype=np.uint32))
                else:
                    pt.do_pass(fb.data_ptr(), p)
        torch.cuda.synchronize()
        return fb.cpu().numpy()
    finally:
        pt.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bvh", ["wide", "binary"])
@pytest.mark.parametrize("kind", ["thinlens", "orthographic"])
def test_schedules_agree(ctl, dev, kind, bvh):
    """A textured floor (the first hit's partials are read), a rough dielectric, a point light and fog, 80 x 48: the
    persistent kernel, the megakernel, the wavefront schedule, render-ahead windows, ctl_render_passes over the three
    passes, block-list passes over every block and the sum of a 2-rank shard give one framebuffer, bit for bit."""
    s = SC.schedule_scene(ctl, kind, SW, SH)
    d = s.compile()
    assert d.sensor and d.n_volumes == 1 and d.n_textures == 1
    if bvh == "binary":
        d = binary_bvh(d)
    base = _schedule(ctl, d, dev)
    assert np.isfinite(base).all() and (base[:, 6] > 0).sum() > 0.9 * SW * SH and base[:, :3].max() > 0
    for name, kw in (("megakernel", dict(flags=ctl.CTL_PT_MEGAKERNEL)), ("wavefront", dict(flags=ctl.CTL_PT_WAVEFRONT)),
                     ("render-ahead", dict(flags=ctl.CTL_PT_RENDER_AHEAD)), ("render_passes", dict(mode="render_passes")),
                     ("blocks", dict(mode="blocks"))):
        got = _schedule(ctl, d, dev, **kw)
        assert same(base, got), (kind, name, first_differences(got, base, SW))
    acc = _schedule(ctl, d, dev, ranks=2, rank=0) + _schedule(ctl, d, dev, ranks=2, rank=1)
    assert same(acc, base), (kind, "2 ranks", first_differences(acc, base, SW))
    # and the sensor is seen: the perspective view of the same room differs
    s0 = SC.schedule_scene(ctl, None, SW, SH)        # (kept: the host scene owns the description's arrays)
    d0 = s0.compile()
    persp = _schedule(ctl, binary_bvh(d0) if bvh == "binary" else d0, dev)
    assert (persp[:, :3] != base[:, :3]).any(axis=1).sum() > SW * SH // 2


# ---------------------------------------------------------------------------------------------
def _three(ctl, d, dev, w=W, h=H):
    """One description through the three integrators: two PathTracer passes, one WPT pass, one PrimTracer pass"""
    out = []
    pt = ctl.PathTracer(0, max_path_length=6)
    try:
        pt.upload_scene(d)
        fb = _fb(dev, w, h)
        for p in range(2):
            pt.do_pass(fb.data_ptr(), p)
        torch.cuda.synchronize()
        out.append(fb.cpu().numpy())
    finally:
        pt.close()
    for t, kw in ((ctl.WavefrontPathTracer(0, max_path_length=6), dict(new_trace=True)), (ctl.PrimTracer(0, draw_mode="first_f_direct"), {})):
        try:
            t.upload_scene(d)
            fb = _fb(dev, w, h)
            t.do_pass(fb.data_ptr(), 0, **kw)
            torch.cuda.synchronize()
            out.append(fb.cpu().numpy())
        finally:
            t.close()
    return out


@pytest.mark.gpu
def test_perspective_is_untouched(ctl, dev):
    """No record and an explicit type-2 record: one framebuffer in every integrator (the first is what the existing
    tests hold to the oracle).  Fields a perspective sensor does not read change nothing."""
    s0 = SC.schedule_scene(ctl, None, SW, SH)
    d0 = s0.compile()
    s2 = SC.schedule_scene(ctl, "perspective", SW, SH)
    d2 = s2.compile()
    assert not d0.sensor and d2.sensor[0].type == 2 and bytes(d0.camera) == bytes(d2.camera)
    a, b = _three(ctl, d0, dev, SW, SH), _three(ctl, d2, dev, SW, SH)
    for name, x, y in zip(("PathTracer", "WavefrontPathTracer", "PrimTracer"), a, b):
        assert same(x, y), (name, first_differences(y, x, SW))
        assert x[:, :3].max() > 0
    d2.sensor[0].aperture_radius = 0.5
    d2.sensor[0].focus_distance = 2.0
    c = _three(ctl, d2, dev, SW, SH)
    assert all(same(x, y) for x, y in zip(a, c))


@pytest.mark.gpu
@pytest.mark.parametrize("fog", [False, True])
def test_a_pinhole_thin_lens_renders_the_perspective_image(ctl, dev, fog):
    """A thin lens of radius 0 focused on the near plane (focus_distance = near = 1, where nearP.z is exactly 1)
    has the perspective sensor's ray, rayX and rayY bit for bit: the lens point is 0 and the focal scale 1.  The
    scene then runs kShadeSensors where the perspective one runs kShadeLights (no fog) or kShadeMedia (fog), and
    must give the same framebuffers bit for bit in every integrator and schedule: the level's first-hit partials
    (the textured floor reads them; sensor_partials from the stored pixel sample), its camera stages, and, without
    fog, the claim that the level's medium code does nothing and draws nothing for a scene without a medium."""
    s0 = SC.schedule_scene(ctl, None, SW, SH, fog=fog)
    d0 = s0.compile()
    s1 = SC.schedule_scene(ctl, None, SW, SH, fog=fog)
    s1.set_sensor("thinlens", aperture_radius=0.0, focus_distance=1.0)
    d1 = s1.compile()
    assert d1.sensor[0].type == 3 and d1.n_volumes == (1 if fog else 0) and d1.n_textures == 1
    q = SC.random_queries(ctl, True, 1024, SW, SH)
    assert ctl.host_sensor_eval(d0, q).tobytes() == ctl.host_sensor_eval(d1, q).tobytes()
    a, b = _three(ctl, d0, dev, SW, SH), _three(ctl, d1, dev, SW, SH)
    for name, x, y in zip(("PathTracer", "WavefrontPathTracer", "PrimTracer"), a, b):
        assert x[:, :3].max() > 0 and same(x, y), (name, first_differences(y, x, SW))
    for flags in (ctl.CTL_PT_MEGAKERNEL, ctl.CTL_PT_WAVEFRONT):
        x, y = _schedule(ctl, d0, dev, flags=flags), _schedule(ctl, d1, dev, flags=flags)
        assert same(x, y), (flags, first_differences(y, x, SW))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["thinlens", "orthographic"])
def test_first_hit_partials_are_the_sensors_ray_differentials(ctl, dev, kind):
    """The PathTracer's first-hit partials against the PrimTracer's, which carries the real rayX and rayY from its
    camera stage.  Both run on the same rays: caller-uploaded sampler tables put the pixel jitter at 0 and the same
    aperture sample per pixel into 2-D draw 1 for the PathTracer and into draw 0 for the PrimTracer.  A tiled
    64 x 64 noise texture (trilinear) on a slanted floor under one grey point light, MaxPathLength 1:
        PathTracer pixel = R / pi * I cos(theta) / d^2          (the light sample; its pdf and pick are 1)
        PrimTracer first_f = R / pi
    with R the filtered texture value, a function of the partials.  The ratio is held to I cos(theta) / d^2,
    float64 from the host evaluator's ray.  Under the thin lens (radius 0.15, focus 2, the floor about 4 away) a
    lens point other than the path's moves rayX's hit by about the pixel footprint itself, |a' - a| |1 - z / f|
    = 0.09 against 0.08, which shifts the MIP level; under the orthographic sensor rayX with the ray's own origin
    has no footprint at all.
    Tolerance 1e-4 relative: under 100 fp32 roundings from the ray to the pixel on either side, 6e-6, and the
    cancellation in light - hit point, conditioned by at most 3 / 1; pixels whose ray meets the floor within 1e-3
    of its rim are left out."""
    s = SC.textured_floor_scene(ctl, kind, **({"aperture_radius": 0.15, "focus_distance": 2.0} if kind == "thinlens" else {}))
    d = s.compile()
    n = W * H
    rng = np.random.default_rng(9)
    ap = rng.random((n, 2)).astype(np.float32)
    ap[0] = 0
    L = ctl.lib()
    pt, pr = ctl.PathTracer(0, max_path_length=1), ctl.PrimTracer(0, draw_mode="first_f")
    try:
        fbs = []
        for t, row in ((pt, 1), (pr, 0)):
            t.upload_scene(d)
            s1, s2 = SC.aperture_tables(row, ap)
            assert L.ctl_sampler_upload(t._ctx, s1.ctypes.data, s2.ctypes.data, 4096, 30, None) == 0
            fb = _fb(dev)
            if t is pt:
                t.render_pass(fb.data_ptr())
            else:
                assert L.ctl_prim_pass(t._ctx, C.byref(t.params), fb.data_ptr(), None, None) == 0
            torch.cuda.synchronize()
            fbs.append(fb.cpu().numpy())
    finally:
        pt.close()
        pr.close()
    got, ref = fbs
    py, px = [a.ravel() for a in np.mgrid[0:H, 0:W]]
    r = ctl.host_sensor_eval(d, SC.queries(ctl, np.stack([px, py], 1).astype(np.float32), ap, True))
    o, dr = r["o"].astype(np.float64), r["d"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t_hit = -o[:, 1] / dr[:, 1]
    P = o + t_hit[:, None] * dr
    inside = (dr[:, 1] < 0) & (np.abs(P[:, 0]) < 3.0 - 1e-3) & (np.abs(P[:, 2]) < 3.0 - 1e-3)
    to_l = np.array(SC.FLOOR_LIGHT[0]) - P
    dist = np.linalg.norm(to_l, axis=1)
    G = SC.FLOOR_LIGHT[1][0] * (to_l[:, 1] / dist) / dist ** 2
    ok = inside & (got[:, 6] == 1) & (ref[:, 6] == 1)
    assert ok.sum() >= n // 2 and (ref[ok, :3] > 0).all()
    assert len(np.unique(ref[ok, 0])) > ok.sum() // 2                          # the texture is seen, pixel by pixel
    want = ref[ok, :3].astype(np.float64) * G[ok, None]
    err = np.abs(got[ok, :3].astype(np.float64) - want) / want
    print(f"{kind}: {int(ok.sum())} pixels, worst relative error {err.max():.3e} (tolerance 1e-4)")
    assert err.max() <= 1e-4


# ---------------------------------------------------------------------------------------------
def _second_pass(ctl, dev, first, updates=()):
    """Pass 0 under `first`, then each description of `updates` through ctl_scene_update(dirty = 0), then pass 1"""
    pt = ctl.PathTracer(0, max_path_length=6)
    try:
        pt.upload_scene(first)
        a, b = _fb(dev, SW, SH), _fb(dev, SW, SH)
        pt.do_pass(a.data_ptr(), 0)
        for d in updates:
            pt.update_scene(d, 0)
        pt.do_pass(b.data_ptr(), 1)
        torch.cuda.synchronize()
        return b.cpu().numpy()
    finally:
        pt.close()


@pytest.mark.gpu
def test_refocusing_and_switching_the_sensor_are_scene_updates(ctl, dev):
    near = SC.schedule_scene(ctl, "thinlens", SW, SH)
    d_near = near.compile()
    far = SC.schedule_scene(ctl, "thinlens", SW, SH)
    d_far = far.compile()
    d_far.sensor[0].focus_distance = 1.25
    d_far.sensor[0].aperture_radius = 0.2
    persp = SC.schedule_scene(ctl, None, SW, SH)
    d_persp = persp.compile()
    fresh_far, fresh_near, fresh_persp = (_second_pass(ctl, dev, d) for d in (d_far, d_near, d_persp))
    assert not same(fresh_far, fresh_near) and not same(fresh_near, fresh_persp)
    got = _second_pass(ctl, dev, d_near, [d_far])
    assert same(got, fresh_far), first_differences(got, fresh_far, SW)
    got = _second_pass(ctl, dev, d_persp, [d_near])
    assert same(got, fresh_near), first_differences(got, fresh_near, SW)
    got = _second_pass(ctl, dev, d_persp, [d_near, d_persp])
    assert same(got, fresh_persp), first_differences(got, fresh_persp, SW)
    # HostScene.set_sensor on the compiled scene: the description as a fresh compile's, handed to the update
    persp.set_sensor("orthographic")
    ortho = SC.schedule_scene(ctl, "orthographic", SW, SH)
    fresh_ortho = _second_pass(ctl, dev, ortho.compile())
    persp2 = SC.schedule_scene(ctl, None, SW, SH)
    got = _second_pass(ctl, dev, persp2.compile(), [d_persp])
    assert same(got, fresh_ortho), first_differences(got, fresh_ortho, SW)


@pytest.mark.gpu
def test_a_refused_update_leaves_the_scene_whole(ctl, dev):
    """Each bad field: the update (and an upload) is refused with a message naming it, and the next pass is the
    one the scene renders without the attempt."""
    s = SC.schedule_scene(ctl, "thinlens", SW, SH)
    d = s.compile()
    want = _second_pass(ctl, dev, d)
    keep = d.sensor
    pt = ctl.PathTracer(0, max_path_length=6)
    try:
        pt.upload_scene(d)
        a = _fb(dev, SW, SH)
        pt.do_pass(a.data_ptr(), 0)
        for field, fields, match in BAD_FIELDS:
            rec = bad_record(ctl, fields)
            d.sensor = C.pointer(rec)
            with pytest.raises(ctl.CTLError, match=match):
                pt.update_scene(d, 0)
            d.sensor = keep
            b = _fb(dev, SW, SH)
            pt.do_pass(b.data_ptr(), 1)
            torch.cuda.synchronize()
            got = b.cpu().numpy()
            assert same(got, want), (field, fields, first_differences(got, want, SW))
        fresh = ctl.PathTracer(0)
        try:
            d.sensor = C.pointer(bad_record(ctl, BAD_FIELDS[0][1]))
            with pytest.raises(ctl.CTLError, match="type"):
                fresh.upload_scene(d)
        finally:
            d.sensor = keep
            fresh.close()
    finally:
        pt.close()
