"""Scenes, sensor settings, query sets and the pass's work order shared by the sensor tests
(test_sensors_host.py on the CPU, test_gpu_sensors.py on the GPU)."""
import numpy as np

import sensor_ref as SR

F = np.float32
W, H = 48, 32                      # one partial 64-pixel tile, aspect != 1
KINDS = ("spherical", "perspective", "thinlens", "orthographic", "telecentric")
NEW_KINDS = ("spherical", "thinlens", "orthographic", "telecentric")
# forward = (-0.4, 0, 4) / |.| is perpendicular to up, so toWorld is a rotation and a translation
CAM = dict(pos=(0.3, 0.2, -4.0), target=(-0.1, 0.2, 0.0), up=(0.0, 1.0, 0.0), fov=50.0)
# the quad of the replay tests stands 4 in front of the camera: thin lens and telecentric focus at 2.5, off it
SENSORS = {
    "spherical": dict(),
    "perspective": dict(),
    "thinlens": dict(aperture_radius=0.15, focus_distance=2.5),
    "orthographic": dict(),
    "telecentric": dict(aperture_radius=0.1, focus_distance=2.5, screen_scale=(1.25, 0.8)),
}
QUAD_L = (3.0, 2.0, 1.5)
QUAD_X1, QUAD_LO, QUAD_HI = 0.35, -40.0, 40.0      # the quad: x in [-40, 0.35], y in [-40, 40] at z = 0, facing -z


def set_camera(s, w=W, h=H):
    s.set_camera(CAM["pos"], CAM["target"], CAM["up"], CAM["fov"], w, h)


# The scene in which the orthographic sensor's two origins decide the image: the camera looks along +z from
# z = -4 with near = 1, and the quad stands at camera-space z = 0.5.  sampleRay starts on z = 0 and sees it;
# sampleRayDifferential starts at nearP, z = 1, behind it.
NEAR_CAM = dict(pos=(0.3, 0.2, -4.0), target=(0.3, 0.2, 0.0), up=(0.0, 1.0, 0.0), fov=50.0)
NEAR_QUAD_Z = -3.5


def quad_scene(ctl, kind, w=W, h=H, sensor=True, quad_z=0.0, cam=None, **over):
    """One emissive black quad of radiance QUAD_L facing the camera, nothing else: about half of every sensor's
    image.  sensor=False leaves the description without a record (the perspective sensor)."""
    s = ctl.HostScene()
    v = np.array([(QUAD_LO, QUAD_LO, quad_z), (QUAD_LO, QUAD_HI, quad_z), (QUAD_X1, QUAD_HI, quad_z),
                  (QUAD_X1, QUAD_LO, quad_z)], F)
    m = s.add_mesh(v, np.array([(0, 1, 2), (0, 2, 3)], np.uint32), [ctl.diffuse_material(0.0, 0.0, 0.0, two_sided=False)])
    node = s.add_node(m)
    s.add_area_light(node, 0, QUAD_L)
    c = cam or CAM
    s.set_camera(c["pos"], c["target"], c["up"], c["fov"], w, h)
    if sensor:
        s.set_sensor(kind, **dict(SENSORS[kind], **over))
    return s, s.compile()


def near_quad_scene(ctl, w=W, h=H):
    return quad_scene(ctl, "orthographic", w, h, quad_z=NEAR_QUAD_Z, cam=NEAR_CAM)


def quad_hit(o, d, quad_z=0.0):
    """Float64: does the ray (o, d) see the quad's front, and how far (relative to the hit point's size) is the hit
    from the quad's edges.  A ray that does not reach the quad's plane from the front is a miss with margin 1: to hit
    the quad a ray from the camera's side needs d.z >= 4 / 57 (the quad's far corner), far from any rounding."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (quad_z - o[:, 2]) / d[:, 2]
    front = (d[:, 2] > 0) & (t > 0)
    p = o + np.where(front, t, 0.0)[:, None] * d
    edge = np.minimum.reduce([np.abs(p[:, 0] - QUAD_X1), np.abs(p[:, 0] - QUAD_LO), np.abs(p[:, 1] - QUAD_LO),
                              np.abs(p[:, 1] - QUAD_HI)]) / (1.0 + np.abs(p).max(axis=1))
    inside = (p[:, 0] < QUAD_X1) & (p[:, 0] > QUAD_LO) & (p[:, 1] > QUAD_LO) & (p[:, 1] < QUAD_HI)
    margin = np.where(front, edge, 1.0)
    return front & inside, margin


def queries(ctl, pX, ap, differential):
    q = np.zeros(len(pX), ctl.SENSOR_QUERY_DTYPE)
    q["pixel_sample"], q["aperture_sample"], q["differential"] = pX, ap, 1 if differential else 0
    return q


def random_queries(ctl, differential, n=4096, w=W, h=H, seed=0):
    rng = np.random.default_rng(seed)
    return queries(ctl, (rng.random((n, 2)) * (w, h)).astype(F), rng.random((n, 2)).astype(F), differential)


def edge_queries(ctl, differential, w=W, h=H):
    """Aperture sample exactly (0.5, 0.5); the disk's branch boundaries after the remap 2 u - 1 (|a| = |b| in all
    four sign pairs, a = b = 0, one of them 0); pixel samples at the four image corners and at (w / 2, h / 2)."""
    aps = [(0.5, 0.5), (0.75, 0.75), (0.25, 0.75), (0.75, 0.25), (0.25, 0.25), (1.0, 1.0), (0.0, 0.0), (0.5, 0.75),
           (0.75, 0.5), (0.5, 0.0), (0.0, 0.5), (0.3, 0.9)]
    pxs = [(0.0, 0.0), (float(w), 0.0), (0.0, float(h)), (float(w), float(h)), (w / 2.0, h / 2.0), (7.25, 19.5)]
    pX = np.array([p for p in pxs for _ in aps], F)
    ap = np.array([a for _ in pxs for a in aps], F)
    return queries(ctl, pX, ap, differential)


def work_order(w, h, tile=64, num_ranks=1, rank=0):
    """work_pixel of the pass (common.h) restated: per owned tile (row-major tiles, tile % num_ranks == rank), the
    tile's 8 x 8 pixel groups row-major, a group's pixels row-major.  (px, py, inside the image) per work item."""
    tx, ty = -(-w // tile), -(-h // tile)
    k = np.arange(tile * tile)
    grp, lane = k // 64, k % 64
    gpr = tile // 8
    ox, oy = (grp % gpr) * 8 + lane % 8, (grp // gpr) * 8 + lane // 8
    px, py = [], []
    for t in range(tx * ty):
        if t % num_ranks == rank:
            px.append((t % tx) * tile + ox)
            py.append((t // tx) * tile + oy)
    px, py = np.concatenate(px), np.concatenate(py)
    return px, py, (px < w) & (py < h)


def draw2(table, idx, nseq=4096):
    """SequenceSampler's 2-D draw for the paths of pixel indices idx, from one draw's row of the 2-D table
    (nseq float2): the fraction of the fp32 sum of sequences idx % nseq and (idx / nseq) % nseq."""
    a, b = idx % nseq, (idx // nseq) % nseq
    v = (F(0) + table[a]) + table[b]
    return (v - np.floor(v)).astype(F)


def schedule_scene(ctl, kind, w=80, h=48, fog=True):
    """An image-textured diffuse floor (the partials are read), a rough dielectric card, an area light, a point
    light and (fog) fog over room and camera, 80 x 48: a second tile column."""
    import media_cases as MC
    from materials_scenes import Mesh
    s = ctl.HostScene()
    rng = np.random.default_rng(5)
    tex = s.add_texture((rng.integers(60, 250, size=(16, 16)).astype(np.uint32) * 0x010101 | 0xff000000).astype(np.uint32),
                        filter=ctl._abi.CTL_TEX_BILINEAR)
    mats = [ctl.diffuse_material(0.6, 0.6, 0.55, texture=tex), ctl.diffuse_material(0.7, 0.7, 0.7),
            ctl.diffuse_material(0.8, 0.8, 0.8), ctl.roughdielectric_material(1, 1.5, 0.25)]
    m = Mesh()
    (x0, y0, z0), (x1, y1, z1) = (-3.0, 0.0, -3.0), (3.0, 4.0, 3.0)
    m.quad([(x0, y0, z0), (x0, y0, z1), (x1, y0, z1), (x1, y0, z0)], 0)   # floor (textured)
    m.quad([(x0, y1, z0), (x1, y1, z0), (x1, y1, z1), (x0, y1, z1)], 1)   # ceiling
    m.quad([(x0, y0, z0), (x0, y1, z0), (x0, y1, z1), (x0, y0, z1)], 1)
    m.quad([(x1, y0, z0), (x1, y0, z1), (x1, y1, z1), (x1, y1, z0)], 1)
    m.quad([(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0)], 1)
    m.quad([(x0, y0, z1), (x0, y1, z1), (x1, y1, z1), (x1, y0, z1)], 1)
    m.quad([(-0.4, 3.9, -0.4), (0.4, 3.9, -0.4), (0.4, 3.9, 0.4), (-0.4, 3.9, 0.4)], 2)    # light, facing down
    m.quad([(-0.9, 0.05, 0.6), (-0.9, 1.4, 1.2), (0.9, 1.4, 1.2), (0.9, 0.05, 0.6)], 3)    # card
    node = s.add_node(m.add_to(s, mats))
    s.add_area_light(node, 2, (14.0, 14.0, 14.0))
    s.add_point_light((1.5, 2.5, -1.0), (3.0, 2.5, 2.0))
    s.set_camera((0.3, 1.2, -2.75), (0.0, 1.2, 0.0), (0, 1, 0), 60.0, w, h)
    if fog:
        MC.add_volume(s, MC.FOG)
    if kind is not None:
        s.set_sensor(kind, **{"thinlens": dict(aperture_radius=0.05, focus_distance=3.0)}.get(kind, {}))
    return s


def ref_rays(desc, q):
    """sensor_ref's float64 rays for a query set: (o, d, oX, dX, oY, dY), None where undefined"""
    cam, S = SR.camera(desc), SR.sensor(desc)
    pX, ap = q["pixel_sample"].astype(np.float64), q["aperture_sample"].astype(np.float64)
    if q["differential"][0]:
        return SR.sample_ray_differential(cam, S, pX, ap)
    return SR.sample_ray(cam, S, pX, ap) + (None, None, None, None)


# ---------------------------------------------------------------------------------------------
# The replay of the quad render: every path's ray from the pass's own samples, through the host evaluator.
MARGIN = 1e-4      # rays left out: a hit closer than this to an edge of the quad (relative to 1 + |hit point|).
                   # The fp32 ray is within 40 * 2^-24 = 2.4e-6 of the exact
                   # one in direction and relative origin (test_sensors_host.py), which moves the hit point by that times
                   # the distance: under 1e-5 of 1 + |hit point|; the traversal's fp32 intersection adds a few 1e-7.


def host_draws(ctl, pass_index, draws=2, nseq=4096, length=30):
    """Rows 0 .. draws - 1 of the pass's 2-D sampler table (ctl_host_sampler_tables): [draw][sequence] float2"""
    s1, s2 = np.zeros(nseq * length, F), np.zeros(nseq * length * 2, F)
    assert ctl.lib().ctl_host_sampler_tables(pass_index, nseq, length, s1.ctypes.data, s2.ctypes.data) == 0
    return s2.reshape(length, nseq, 2)[:draws]


def replay(ctl, desc, integrator, draws, w=W, h=H, quad_z=0.0):
    """The paths of one pass over desc's quad scene: per path the query it makes of the sensor (q), the pixel
    index its sample is added to (pixel; -1: off the image), and from the host evaluator's ray intersected with
    the quad in float64 whether it sees the quad (hit) and whether it is left out (skip, MARGIN).
      "pt"    PathTracer: work order; pixel sample (px, py) + draw 0, aperture draw 1, sampleRayDifferential; the
              sample lands on floor(pixel sample)
      "wpt"   WavefrontPathTracer: pixel order; the same draws through sampleRay; lands on its own pixel
      "prim"  PrimTracer: pixel order; the unjittered pixel, aperture draw 0, sampleRayDifferential; its own pixel"""
    if integrator == "pt":
        px, py, inside = work_order(w, h)
        px, py = px[inside], py[inside]
    else:
        py, px = [a.ravel() for a in np.mgrid[0:h, 0:w]]
    idx = py * w + px
    xy = np.stack([px, py], 1).astype(F)
    if integrator == "prim":
        pX, ap = xy, draw2(draws[0], idx)
    else:
        pX, ap = xy + draw2(draws[0], idx), draw2(draws[1], idx)
    q = queries(ctl, pX, ap, integrator != "wpt")
    r = ctl.host_sensor_eval(desc, q)
    hit, margin = quad_hit(r["o"], r["d"], quad_z)
    if integrator == "pt":
        lx, ly = np.floor(pX[:, 0]).astype(np.int64), np.floor(pX[:, 1]).astype(np.int64)
        pixel = np.where((lx < w) & (ly < h), ly * w + lx, -1)
    else:
        pixel = idx
    return dict(q=q, rays=r, pixel=pixel, hit=hit, skip=margin < MARGIN)


def expected_image(rp, w=W, h=H):
    """(rgb, weight, usable) per pixel: the samples of the replay's hits added as AddSample adds them (QUAD_L per
    hit, 0 per miss, weight 1 each; equal addends, so their order does not matter); a pixel that a left-out ray
    landed on is not usable."""
    n = w * h
    on = rp["pixel"] >= 0
    weight = np.bincount(rp["pixel"][on], minlength=n)
    hits = np.bincount(rp["pixel"][on & rp["hit"]], minlength=n)
    usable = np.bincount(rp["pixel"][on & rp["skip"]], minlength=n) == 0
    rgb = np.zeros((n, 3), F)
    for k in range(1, int(hits.max()) + 1):
        rgb[hits >= k] += np.array(QUAD_L, F)
    return rgb, weight.astype(F), usable


# ---------------------------------------------------------------------------------------------
# The floor of the partials test: a tiled high-frequency texture under one point light, seen at a slant.
FLOOR_LIGHT = ((0.0, 3.0, 0.0), (8.0, 8.0, 8.0))      # position, grey intensity


def textured_floor_scene(ctl, kind, w=W, h=H, **sensor):
    from materials_scenes import Mesh
    s = ctl.HostScene()
    rng = np.random.default_rng(11)
    img = rng.integers(20, 255, size=(64, 64, 3)).astype(np.uint32)
    tex = s.add_texture((img[..., 0] | (img[..., 1] << 8) | (img[..., 2] << 16) | 0xff000000).astype(np.uint32),
                        mapping=(4.0, 0.0, 0.0, 0.0, 4.0, 0.0))                 # trilinear, tiled 4 x 4
    m = Mesh()
    m.quad([(-3.0, 0.0, -3.0), (-3.0, 0.0, 3.0), (3.0, 0.0, 3.0), (3.0, 0.0, -3.0)], 0)     # facing up
    s.add_node(m.add_to(s, [ctl.diffuse_material(0.9, 0.9, 0.9, texture=tex)]))
    s.add_point_light(*FLOOR_LIGHT)
    s.set_camera((0.3, 2.0, -3.5), (0.0, 0.0, 0.0), (0, 1, 0), 50.0, w, h)
    s.set_sensor(kind, **sensor)
    return s


def aperture_tables(row, aperture, seed=2, nseq=4096, length=30):
    """Sampler tables (1-D, 2-D; element-major) whose 2-D draw `row` is aperture[i] for the path of pixel index i
    < nseq and whose 2-D draws below `row` are 0: sequence 0 holds 0 in those rows, so the fraction of the sum of
    sequences i and 0 is the entry itself."""
    rng = np.random.default_rng(seed)
    s1 = rng.random((length, nseq)).astype(F)
    s2 = rng.random((length, nseq, 2)).astype(F)
    s2[:row + 1] = 0
    s2[row, 1:len(aperture)] = aperture[1:]
    return s1, s2
