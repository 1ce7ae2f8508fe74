"""One homogeneous participating medium on the GPU: the batch medium entry against its host twin bit for
bit, what upload and update refuse, renders that a medium out of reach leaves untouched, an absorbing
medium and a white furnace with closed forms, the schedules of the PathTracer against each other, and the
volume changed by ctl_scene_update.  Images are 64 x 64; no test hands the oracle a scene with a volume."""
import numpy as np
import pytest
import torch

import light_cases as LC
import media_cases as MC
from helpers import binary_bvh
from materials_scenes import Mesh, first_differences, same, uniform_env, ENV_RGB
from test_gpu_lights import (W, H, REL, _fb, check_render, expected_samples, pass_rays, render_pt, same_records,
                             with_neighbours)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def device_medium_eval(ctl, t, q, dev):
    dq = torch.from_numpy(np.frombuffer(q.tobytes(), np.uint8).copy()).to(dev)
    dr = torch.zeros(len(q) * ctl.MEDIUM_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    t.medium_eval(len(q), dq.data_ptr(), dr.data_ptr())
    torch.cuda.synchronize()
    return np.frombuffer(dr.cpu().numpy().tobytes(), dtype=ctl.MEDIUM_RESULT_DTYPE)


# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_evaluator_equals_the_host_evaluator_bit_for_bit(ctl, dev):
    """ctl_medium_eval (HIP) against ctl_host_medium_eval on every set of the host tests: the random sets,
    the edge rays, and every op with NaNs and infinities in each input; and on a scene without a volume."""
    by_volume = {}
    for name, op, q, _ in MC.random_sets(ctl):
        by_volume.setdefault(name, []).append((op, q))
    for op in ("intersect", "transmittance"):
        for name, (q, *_) in MC.edge_rays(ctl, op).items():
            by_volume["axis_iso"].append((f"{op} {name}", q))
    for name in ("axis_iso", "empty_channel", "tilted_hg"):
        by_volume[name].append(("nan", MC.nan_queries(ctl)))
    by_volume[None] = [("no volume", MC.op_set(ctl, "axis_iso", "transmittance", 64)[0])]
    t = ctl.Tracer(0)
    try:
        for name, sets in by_volume.items():
            _, desc = MC.eval_scene(ctl, name)
            t.upload_scene(desc)
            for what, q in sets:
                got, want = device_medium_eval(ctl, t, q, dev), ctl.host_medium_eval(desc, q)
                bad = same_records(got, want)
                assert bad.size == 0, (name, what, len(bad), q[bad[0]], got[bad[0]], want[bad[0]])
    finally:
        t.close()


def _room_like(ctl, volume=None, vol_over=None):
    s, _ = LC.mixed_host_scene(ctl)
    if volume is not None:
        MC.add_volume(s, volume, **(vol_over or {}))
    return s


# A box no camera, bounce or shadow ray of the mixed scene can reach: the scene lies in y >= 0 (the floor
# spans |x|, |z| <= 6 at y = 0, everything else is above it), the camera looks down on it, and every ray
# that leaves the scene goes to the environment from y >= 0 upwards or, below the floor's rim, downwards
# from outside |x|, |z| <= 6 -- the box hangs under the middle of the floor, inside the floor's shadow cone
# for every origin on or above the floor.
FAR_BOX = MC.trs((1.0, 1.0, 1.0), (-0.5, -3.0, -0.5))


@pytest.mark.gpu
def test_upload_and_update_refuse_malformed_volumes(ctl, dev):
    A = ctl._abi
    V = MC.VOLUMES["tilted_hg"]
    s = _room_like(ctl, V)
    d = s.compile()
    r = d.volumes[0]
    nan, inf = float("nan"), float("inf")
    cases = [("kind", 2, "kind"), ("kind", 0, "kind"), ("phase", 2, "phase"), ("phase_g", 1.0, "below 1"),
             ("phase_g", -1.0, "below 1"), ("phase_g", nan, "non-finite")]
    pt = ctl.PathTracer(0, max_path_length=4)
    try:
        pt.upload_scene(d)
        fb0, fb1 = _fb(dev), _fb(dev)
        pt.do_pass(fb0.data_ptr(), 0)

        def refused(match):
            with pytest.raises(ctl.CTLError, match=match):
                pt.update_scene(d, A.CTL_DIRTY_VOLUMES)
            t = ctl.Tracer(0)
            try:
                with pytest.raises(ctl.CTLError, match=match):
                    t.upload_scene(d)
            finally:
                t.close()

        for field, value, match in cases:
            keep = getattr(r, field)
            setattr(r, field, value)
            try:
                refused(match)
            finally:
                setattr(r, field, keep)
        for arr, value, match in (("sig_a", nan, "non-finite"), ("sig_s", inf, "non-finite"), ("le", nan, "non-finite"),
                                  ("sig_a", -0.5, "negative"), ("sig_s", -1e-3, "negative")):
            a = getattr(r, arr)
            keep = a[1]
            a[1] = value
            try:
                refused(match)
            finally:
                a[1] = keep
        for mat in ("volume_to_world", "world_to_volume"):
            m = getattr(r, mat).m
            keep = m[7]
            m[7] = nan
            try:
                refused("non-finite")
            finally:
                m[7] = keep
        d.n_volumes = 2
        try:
            refused("more than one")
        finally:
            d.n_volumes = 1
        # a changed record without the flag is refused too (the caller forgot CTL_DIRTY_VOLUMES), with any other
        # group or none marked; the unchanged record passes
        keep = r.sig_s[1]
        r.sig_s[1] = keep * 2
        try:
            for dirty in (0, A.CTL_DIRTY_LIGHTS):
                with pytest.raises(ctl.CTLError, match="CTL_DIRTY_VOLUMES"):
                    pt.update_scene(d, dirty)
        finally:
            r.sig_s[1] = keep
        pt.update_scene(d, 0)
        pt.update_scene(d, A.CTL_DIRTY_LIGHTS)
        # the uploaded scene is whole: the same pass again gives the same bits
        pt.do_pass(fb1.data_ptr(), 0)
        torch.cuda.synchronize()
        assert same(fb0.cpu().numpy(), fb1.cpu().numpy())
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------
def _render(ctl, d, dev, params, passes=4):
    pt = ctl.PathTracer(0)
    try:
        pt.upload_scene(d)
        pt.params = params
        fb = _fb(dev)
        for p in range(passes):
            pt.do_pass(fb.data_ptr(), p)
        torch.cuda.synchronize()
        return fb.cpu().numpy(), pt.rays_traced()
    finally:
        pt.close()


@pytest.mark.gpu
def test_a_medium_out_of_reach_changes_nothing(ctl, dev):
    """kShadeMedia against kShadeLights on equal paths: the mixed scene plus a volume under the floor."""
    far = MC.volume(FAR_BOX, (0.5, 0.25, 1.0), (1.0, 2.0, 0.5), "hg", 0.5)
    s0, s1 = _room_like(ctl), _room_like(ctl, far)      # the scenes own the descriptions' arrays
    d0, d1 = s0.compile(), s1.compile()
    assert d0.n_volumes == 0 and d1.n_volumes == 1
    p = ctl.PTParams(1, 8, 3, 1, 64, 1, 0, 0)
    a, ra = _render(ctl, d0, dev, p)
    b, rb = _render(ctl, d1, dev, p)
    assert same(a, b), first_differences(b, a, W)
    assert ra == rb and a[:, :3].max() > 0
    for mode in ("first_f_direct", "first_f"):
        out = []
        for d in (d0, d1):
            t = ctl.PrimTracer(0, draw_mode=mode)
            try:
                t.upload_scene(d)
                fb = _fb(dev)
                t.do_pass(fb.data_ptr(), 0)
                torch.cuda.synchronize()
                out.append(fb.cpu().numpy())
            finally:
                t.close()
        assert same(out[0], out[1]), mode
    # the WavefrontPathTracer never reads the medium: a box across the whole scene changes nothing
    across = MC.volume(MC.trs((16.0, 16.0, 16.0), (-8.0, -8.0, -8.0)), (0.5, 0.25, 1.0), (1.0, 2.0, 0.5))
    s2 = _room_like(ctl, across)
    d2 = s2.compile()
    out = []
    for d in (d0, d2):
        t = ctl.WavefrontPathTracer(0, direct=True, max_path_length=4, rr_start_depth=5)
        try:
            t.upload_scene(d)
            fb = _fb(dev)
            t.do_pass(fb.data_ptr(), 0, new_trace=True)
            torch.cuda.synchronize()
            out.append(fb.cpu().numpy())
        finally:
            t.close()
    assert same(out[0], out[1]) and out[0][:, :3].max() > 0
    # ... while the PathTracer sees it
    c, _ = _render(ctl, d2, dev, p, passes=1)
    a1, _ = _render(ctl, d0, dev, p, passes=1)
    assert not same(a1, c)


# ---------------------------------------------------------------------------------------------
# The absorbing medium: sig_s = 0 makes every albedo 0, so the sampling weight is 0, no distance is ever
# sampled, pdf_failure = 0 * avg(T) + 1 = 1 and a surface behind the medium carries exactly its transmittance.
ABSORB = MC.volume(MC.trs((16.0, 16.0, 16.0), (-8.0, -8.0, -8.0)), (0.125, 0.25, 0.0625), (0.0, 0.0, 0.0))


def _absorbing_scene(ctl):
    s = ctl.HostScene()
    m = Mesh()
    LC.floor_mesh(m)
    s.add_node(m.add_to(s, [ctl.diffuse_material(*LC.RHO)]))
    s.set_camera(LC.CAM["pos"], LC.CAM["target"], LC.CAM["up"], LC.CAM["fov"], W, H)
    LC.add_analytic_light(s, "point")
    MC.add_volume(s, ABSORB)
    return s, s.compile()


def _segment_T(a, b):
    sig = ABSORB["sig_a"].astype(np.float64)
    return np.exp(-np.linalg.norm(np.asarray(b, np.float64) - a, axis=1)[:, None] * sig[None, :])


@pytest.mark.gpu
def test_absorbing_medium_in_the_prim_tracer(ctl, dev):
    """first_f_direct: T(camera -> P) * (direct + rho / 2 pi), the direct term unattenuated.

    Tolerance: the lights test's REL for the surface term, plus the transmittance's own error: the exponent
    sig * L (at most 0.25 * 4.4 = 1.1) carries the distance's few roundings, 1.1 * 4 * 2^-24 < 3e-7,
    inside REL = 1e-4."""
    s, d = _absorbing_scene(ctl)
    ys, xs = np.mgrid[0:H, 0:W]
    sx, sy = xs.ravel().astype(np.float64), ys.ravel().astype(np.float64)
    val, tol, skip, _ = expected_samples("point", d, sx, sy)
    o, dirs = LC.pixel_corner_rays(d, sx, sy)
    T = _segment_T(o[None, :], LC.floor_points(o, dirs))
    base = np.asarray(LC.RHO, np.float64) / (2 * np.pi)
    t = ctl.PrimTracer(0, draw_mode="first_f_direct")
    try:
        t.upload_scene(d)
        fb = _fb(dev)
        t.do_pass(fb.data_ptr(), 0)
        torch.cuda.synchronize()
        got = fb.cpu().numpy()
    finally:
        t.close()
    want = T * (val + base[None, :])
    check_render("prim absorbing", got, want, T * (tol + REL * base[None, :]) + REL * want, skip, np.arange(W * H))


@pytest.mark.gpu
def test_absorbing_medium_in_the_path_tracer(ctl, dev):
    """MaxPathLength 1, Direct 1: the pixel is T(camera -> P) * T(P -> light) times the lights test's value.
    Same tolerance as the PrimTracer's test, with two transmittances."""
    s, d = _absorbing_scene(ctl)
    got, geo = render_pt(ctl, d, dev, ctl.PTParams(1, 1, 5, 1, 64, 1, 0, 0))
    sx, sy, pixel, near = geo
    val, tol, skip, _ = expected_samples("point", d, sx, sy)
    o, dirs = LC.pixel_corner_rays(d, sx, sy)
    P = LC.floor_points(o, dirs)
    T1 = _segment_T(o[None, :], P)
    w = T1
    T2 = _segment_T(P, LC.A_POINT["pos"].astype(np.float64)[None, :])
    skip = skip | np.isin(pixel, with_neighbours(pixel, near))
    want = w * T2 * val
    check_render("pt absorbing", got, want, w * T2 * tol + REL * want, skip, pixel)


# ---------------------------------------------------------------------------------------------
def _furnace_scene(ctl, phase, g, light=None, sig_a=(0.1, 0.1, 0.1), sig_s=(0.4, 0.4, 0.4), env=True, fog=True):
    """Camera inside a box of fog, the only geometry a triangle of area 1e-6 a thousand units behind it."""
    s = ctl.HostScene()
    v = np.array([(0, 0, 1000.0), (0.002, 0, 1000.0), (0, 0.001, 1000.0)], np.float32)
    s.add_node(s.add_mesh(v, np.array([(0, 1, 2)], np.uint32), [ctl.diffuse_material(0.5, 0.5, 0.5)]))
    s.set_camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 60.0, W, H)
    if env:
        uniform_env(s, ctl)
    if light is not None:
        s.add_point_light(*light)
    if fog:
        MC.add_volume(s, MC.volume(MC.trs((8.0, 8.0, 8.0), (-4.0, -4.0, -4.0)), sig_a, sig_s, phase, g))
    return s, s.compile()


@pytest.mark.gpu
@pytest.mark.parametrize("phase,g", [("isotropic", 0.0), ("hg", 0.7)])
def test_white_furnace(ctl, dev, phase, g):
    """A grey medium of albedo 0.8 under a constant environment E, Direct = 0: a scattering event weighs
    sigma_s T / (w avg(sigma_t T)) = 1 with w = albedo, the phase sample 1, leaving the medium is unweighted,
    and a path that ends inside collects E along its last direction: every pixel is E.

    E is the value the same camera sees under the same environment WITHOUT the volume: there every camera ray
    leaves the scene at depth 1 and the pixel is the environment's radiance, through the kShadeEnv kernels and
    the decode and scale the environment tests hold.  That image is constant up to the map lookup's rounding
    (asserted at 1e-6) and in the map's proportions; the furnace's pixels are compared with its level.

    Tolerance: at most 8 events, each a quotient of two products of three factors (8 roundings) and a
    Russian-roulette division past depth 5 (2 more), and E itself a bilinear lookup of a constant map (4):
    8 * 10 + 4 = 84 roundings of 2^-24, 5e-6 relative; 1e-5."""
    s, d = _furnace_scene(ctl, phase, g)
    s0, d0 = _furnace_scene(ctl, phase, g, fog=False)
    clear, clear_rays = _render(ctl, d0, dev, ctl.PTParams(0, 8, 5, 1, 64, 1, 0, 0), passes=1)
    assert clear_rays == W * H
    seen = clear[:, 6] > 0
    cpx = clear[seen, :3].astype(np.float64) / clear[seen, 6:7]
    E = np.median(cpx, axis=0)
    assert E.min() > 0.1 and np.abs(cpx / E[None, :] - 1).max() <= 1e-6
    rgb = np.array(ENV_RGB, np.float64)
    assert np.abs(E / E[0] - rgb / rgb[0]).max() < 1e-5
    base = None
    for flags in (0, ctl.CTL_PT_MEGAKERNEL, ctl.CTL_PT_WAVEFRONT):
        got, rays = _render(ctl, d, dev, ctl.PTParams(0, 8, 5, 1, 64, 1, 0, flags), passes=1)
        n = got[:, 6]
        assert n.sum() == W * H and np.array_equal(n, clear[:, 6])
        lit = n > 0
        px = got[lit, :3].astype(np.float64) / n[lit, None]
        err = np.abs(px / E[None, :] - 1).max()
        print(f"furnace {phase} flags {flags}: worst relative deviation from E = {E.tolist()} {err:.3e}, rays {rays}")
        assert err <= 1e-5
        assert rays > 2 * W * H            # the paths did scatter
        if base is None:
            base = (got, rays)
        else:
            assert same(base[0], got) and base[1] == rays, first_differences(got, base[0], W)


# ---------------------------------------------------------------------------------------------
def _schedule(ctl, d, dev, flags=0, ranks=1, rank=0, mode="do_pass", passes=4):
    pt = ctl.PathTracer(0)
    try:
        pt.upload_scene(d)
        pt.params = ctl.PTParams(1, 8, 3, 1, 16, ranks, rank, flags)
        fb = _fb(dev)
        if mode == "render_passes":
            pt.render_passes(fb.data_ptr(), 0, passes)
        else:
            for p in range(passes):
                if mode == "blocks":
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
def test_schedules_agree_in_the_fog(ctl, dev, bvh):
    s = MC.fog_room(ctl)
    d = s.compile()
    assert d.n_volumes == 1 and d.n_tri_data <= 30
    if bvh == "binary":
        d = binary_bvh(d)
    base, rays = _schedule(ctl, d, dev)
    assert np.isfinite(base).all() and (base[:, 6] > 0).sum() > 0.9 * W * H and base[:, :3].max() > 0
    for name, kw in (("render_passes", dict(mode="render_passes")), ("render-ahead", dict(flags=ctl.CTL_PT_RENDER_AHEAD)),
                     ("megakernel", dict(flags=ctl.CTL_PT_MEGAKERNEL)), ("wavefront", dict(flags=ctl.CTL_PT_WAVEFRONT)),
                     ("blocks", dict(mode="blocks"))):
        got, r = _schedule(ctl, d, dev, **kw)
        assert same(base, got), (name, first_differences(got, base, W))
        if name == "render-ahead":
            # ctl_rays_traced counts a render-ahead window when it is launched (include/ctl_trace.h,
            # CTL_PT_RENDER_AHEAD): the fourth call launches passes 3 .. 6, so after four passes the
            # count holds three passes nobody asked for yet.  Seven passes (1 + 2 + 4) end on a
            # window's edge, and there the counts are equal.
            assert r > rays
            got7, r7 = _schedule(ctl, d, dev, passes=7, **kw)
            base7, rays7 = _schedule(ctl, d, dev, passes=7)
            assert same(base7, got7) and r7 == rays7, (name, r7, rays7)
        else:
            assert r == rays, name
    acc, total = np.zeros_like(base), 0
    for rank in range(3):
        got, r = _schedule(ctl, d, dev, ranks=3, rank=rank)
        acc += got
        total += r
    assert same(acc, base) and total == rays
    s0 = MC.fog_room(ctl, fog=False)
    d0 = s0.compile()
    clear, _ = _schedule(ctl, binary_bvh(d0) if bvh == "binary" else d0, dev)
    differs = (clear[:, :3].view(np.uint32) != base[:, :3].view(np.uint32)).any(axis=1)
    assert differs.sum() > W * H // 2


# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_volume_changes_through_a_scene_update(ctl, dev):
    A = ctl._abi
    thick = dict(MC.FOG, sig_s=MC.f32([0.6, 0.5, 0.4]))
    s0, s1, s2 = MC.fog_room(ctl), MC.fog_room(ctl, fog=False), MC.fog_room(ctl, fog=False)
    MC.add_volume(s1, thick)
    d0, d1, d_clear = s0.compile(), s1.compile(), s2.compile()
    p = ctl.PTParams(1, 6, 3, 1, 64, 1, 0, 0)

    def two_passes(first, second):
        pt = ctl.PathTracer(0)
        try:
            pt.upload_scene(first)
            pt.params = p
            a, b = _fb(dev), _fb(dev)
            pt.do_pass(a.data_ptr(), 0)
            if second is not None:
                pt.update_scene(second, A.CTL_DIRTY_VOLUMES)
            pt.do_pass(b.data_ptr(), 1)
            torch.cuda.synchronize()
            return a.cpu().numpy(), b.cpu().numpy()
        finally:
            pt.close()

    _, b_updated = two_passes(d0, d1)
    _, b_fresh = two_passes(d1, None)
    _, b_unchanged = two_passes(d0, None)
    assert same(b_updated, b_fresh), first_differences(b_updated, b_fresh, W)
    assert not same(b_updated, b_unchanged)
    # the volume removed, and added, by an update: the level changes with it
    _, b_removed = two_passes(d0, d_clear)
    _, b_clear = two_passes(d_clear, None)
    assert same(b_removed, b_clear), first_differences(b_removed, b_clear, W)
    _, b_added = two_passes(d_clear, d0)
    assert same(b_added, b_unchanged), first_differences(b_added, b_unchanged, W)


# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_single_scatter_replay(ctl, dev):
    """MaxPathLength 1, Direct 1, one pass, no environment, a point light behind the camera inside the fog:
    a pixel is the depth-1 medium event alone.  The event is replayed in float64 (media_ref.py, light_ref.py's
    point light formula I / d^2) from the pass's own tables: the path of pixel index i draws its distance from
    1-D draw 0 of sequences i and 0 (their sum's fraction), and its light sample from 2-D draw 2, which a single
    point light does not read (draws 0 and 1 are the sensor's).
        pixel = sigma_s T(t) / pdfSuccess * I / d^2 * T(p -> light) * HG(-dir, d) * 1 / (1 + HG^2)
    (the light's pdf is 1 in the discrete measure, the pick probability 1).  Pixels whose replay did not scatter
    are exactly 0.

    Tolerance, relative: 1e-4 for the under 150 roundings of the event (camera ray, slab test, log, two
    exponentials, the phase function, the products: 9e-6 if all err one way) with the conditioning of the
    lights tests' renders, plus the sampled distance's own error dsd (test_media_host.py: (9 EPS / (1 - u') + 3
    EPS |log(1 - u')|) / sig_t) carried into the point p: 1 / d^2 moves by 2 dsd / d, the phase function's
    cosine by dsd / d with |dHG / dcos| / HG <= 3 g / (1 - g)^2 < 2, and the two transmittances by sig_t dsd
    each: dsd (4 / d + 2 max sig_t).  Left out: the margins of test_media_host.py (u against the sampling
    weight, 3 u / w against a channel boundary, the distance against the box's exit), and the pixels a sample
    near a pixel border may have landed on; at most 2 % in all."""
    import media_ref as MR
    EPS = 2.0 ** -24
    light = (MC.f32([0.5, 0.25, 2.0]), MC.f32([3.0, 2.5, 2.0]))
    sig_a, sig_s, g = (0.05, 0.1, 0.15), (0.3, 0.25, 0.2), 0.3
    s, d = _furnace_scene(ctl, "hg", g, light=light, sig_a=sig_a, sig_s=sig_s, env=False)
    V = MC.volume(MC.trs((8.0, 8.0, 8.0), (-4.0, -4.0, -4.0)), sig_a, sig_s, "hg", g)
    A = ctl._abi
    pt = ctl.PathTracer(0)
    try:
        pt.upload_scene(d)
        pt.params = ctl.PTParams(1, 1, 5, 1, 64, 1, 0, 0)
        sx, sy, pixel, near = pass_rays(ctl, pt, d, dev, 0)
        fb = _fb(dev)
        pt.do_pass(fb.data_ptr(), 0)
        torch.cuda.synchronize()
        got = fb.cpu().numpy()
        nseq = 4096
        s1 = pt.read_array(A.CTL_ARRAY_SAMPLES_1D, 0, nseq, np.float32, 1)[:, 0]      # draw 0 of every sequence
        s2 = pt.read_array(A.CTL_ARRAY_SAMPLES_2D, 2 * nseq, nseq, np.float32, 2)     # draw 2
    finally:
        pt.close()
    n = W * H
    assert n <= nseq and np.isfinite(s2).all()
    # ctl_camera_rays lists the rays in the pass's work order, not by pixel: a ray belongs to the path of the
    # pixel its sample position lies in (px + jitter), unless that position is within 1e-4 of a pixel border or
    # off the image, where the fp32 sum may have rounded over; those rays and their pixels are left out below
    moved = near | (pixel < 0)
    idx = np.where(pixel >= 0, pixel, 0)
    assert np.array_equal(np.sort(idx[~moved]), np.unique(idx[~moved]))      # one path per pixel
    v = s1[idx] + s1[0]                      # a = idx % nseq, b = (idx / nseq) % nseq = 0, summed in fp32
    u = (v - np.floor(v)).astype(np.float32).astype(np.float64)
    o, dirs = LC.pixel_corner_rays(d, sx, sy)
    ori = np.broadcast_to(o, dirs.shape)
    box = MR.intersect(V, ori, dirs, np.zeros(n), np.full(n, MR.FLT_MAX))
    assert box["hit"].all() and not box["t0"].any()
    r = MR.sample_distance(V, ori, dirs, box["t0"], box["t1"], u)
    w, st = r["weight"], r["sig_t"][r["channel"]]
    with np.errstate(divide="ignore", invalid="ignore"):
        dsd = np.where(r["tried"], (9 * EPS / (1 - r["u1"]) + 3 * EPS * np.abs(np.log1p(-r["u1"]))) / st, 0.0)
    frac = r["v"] - np.floor(r["v"])
    skip = np.abs(u - w) <= 1e-6
    skip |= r["tried"] & ~(((frac > 1e-5) & (frac < 1 - 1e-5)) | (r["v"] < 0.5))
    skip |= r["tried"] & (np.abs(r["sd"] - r["span"]) <= dsd + 1e-5 * r["span"] + 1e-5)
    skip |= np.isin(pixel, with_neighbours(pixel, near))
    skip |= moved
    scat = r["success"]
    to_l = light[0].astype(np.float64)[None, :] - r["p"]
    dist = np.linalg.norm(to_l, axis=1)
    wo = to_l / dist[:, None]
    ph, _ = MR.hg(g, np.sum(-dirs * wo, axis=1))
    sig_t = r["sig_t"]
    cf = np.asarray(sig_s, np.float32).astype(np.float64)[None, :] * r["transmittance"] / r["pdf_success"][:, None]
    val = cf * light[1].astype(np.float64)[None, :] / (dist ** 2)[:, None] * np.exp(-dist[:, None] * sig_t[None, :])
    val = val * (ph * (1.0 / (1.0 + ph * ph)))[:, None]
    val = np.where(scat[:, None], val, 0.0)
    rel = 1e-4 + dsd * (4.0 / dist + 2.0 * sig_t.max())
    ok = ~skip
    print(f"replay: scattered {int((scat & ok).sum())}, passed through {int((~scat & ok).sum())}, left out {int(skip.sum())}")
    assert skip.sum() <= 0.02 * n
    assert (scat & ok).sum() >= n // 4 and (~scat & ok).sum() >= n // 4
    got = got[idx]                           # per ray: the pixel its sample landed on
    assert np.all(got[ok, 6] == 1)
    dark = ok & ~scat
    assert not got[dark, :3].any()
    lit = ok & scat
    err = np.abs(got[lit, :3].astype(np.float64) - val[lit])
    lim = rel[lit, None] * val[lit]
    print(f"replay: worst error / tolerance {(err / lim).max():.4f}, worst relative error {(err / val[lit]).max():.3e}")
    assert np.all(err <= lim), float((err / lim).max())
    assert val[lit].max() > 1e-3
