"""Scenes and query sets of the point / spot / distant light tests, shared by test_lights_host.py
(CPU) and test_gpu_lights.py.  Every number that reaches the library is fp32-representable, so the
float64 reference (light_ref.py) and the library start from the same inputs."""
import ctypes as C
import functools

import numpy as np

import light_ref as LR
from materials_scenes import Mesh

F = np.float32
RHO = (0.5, 0.625, 0.75)          # the floor's reflectance, exact in fp32


def f32(a):
    return np.asarray(a, np.float32)


def floor_mesh(m, half=3.0, k=0):
    """Two triangles in the plane z = 0, normal +z (wound so that cross(v1 - v0, v2 - v0) = +z): the one
    axis whose 16-bit spherical code decodes to the axis exactly."""
    m.quad([(-half, -half, 0), (half, -half, 0), (half, half, 0), (-half, half, 0)], k)


def queries(ctl, light, ref, ref_n=(0.0, 0.0, 1.0), sample=None):
    ref = f32(ref).reshape(-1, 3)
    q = np.zeros(ref.shape[0], ctl.LIGHT_QUERY_DTYPE)
    q["light"] = light
    q["ref"] = ref
    q["ref_n"] = f32(ref_n)
    if sample is not None:
        q["sample"] = f32(sample)
    return q


# ---------------------------------------------------------------------------------------------
# The evaluator scene: a floor and five delta lights.  Spots: the narrowest cutoff (10 degrees) with
# the narrowest band (2 degrees), a middle one, a wide one.
POINT = dict(pos=f32([0.75, 1.5, -0.5]), I=f32([3.0, 2.0, 1.5]))
SPOTS = [dict(pos=f32([0.5, 2.0, 0.25]), target=f32([1.5, -1.0, 2.75]), I=f32([5.0, 4.0, 3.0]), cutoff=F(10.0), beam=F(8.0)),
         dict(pos=f32([-1.0, 1.25, 0.5]), target=f32([1.0, -2.0, -2.0]), I=f32([2.0, 2.5, 3.0]), cutoff=F(40.0), beam=F(25.0)),
         dict(pos=f32([0.25, -1.5, 1.0]), target=f32([-2.5, 1.5, -1.0]), I=f32([1.0, 0.5, 0.25]), cutoff=F(75.0), beam=F(30.0))]
DISTANT = dict(E=f32([1.5, 1.25, 1.0]), dir=f32([0.5, 2.0, -1.0]), r=F(0.75))
I_POINT, I_SPOT0, I_DISTANT = 0, 1, 4     # light indices in eval_scene


@functools.lru_cache(maxsize=None)
def _eval_scene(ctl):
    s = ctl.HostScene()
    m = Mesh()
    floor_mesh(m)
    s.add_node(m.add_to(s, [ctl.diffuse_material(*RHO)]))
    s.set_camera((0, 0, 4), (0, 0, 0), (0, 1, 0), 40.0, 64, 64)
    assert s.add_point_light(POINT["pos"], POINT["I"]) == I_POINT
    for k, sp in enumerate(SPOTS):
        assert s.add_spot_light(sp["pos"], sp["target"], sp["I"], sp["cutoff"], sp["beam"]) == I_SPOT0 + k
    assert s.add_distant_light(DISTANT["E"], DISTANT["dir"], DISTANT["r"]) == I_DISTANT
    return s, s.compile()


def eval_scene(ctl):
    return _eval_scene(ctl)


def _well_conditioned(p, ref):
    """|p - ref| >= max(|p|, |ref|) / 8: the subtraction p - ref loses at most a factor 16."""
    n = np.linalg.norm
    return n(p - ref, axis=1) >= np.maximum(n(p, axis=1), n(ref, axis=1)) / 8.0


def _ball(rng, n, radius):
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v * (radius * rng.random(n) ** (1.0 / 3.0))[:, None]


def point_refs(n=4096, seed=1):
    rng = np.random.default_rng(seed)
    ref = f32(_ball(rng, 4 * n, 4.0)).astype(np.float64)
    keep = _well_conditioned(np.broadcast_to(POINT["pos"].astype(np.float64), ref.shape), ref)
    assert keep.sum() >= n
    return f32(ref[keep][:n])


def spot_refs(k, n=4096, seed=2):
    """Reference points in a cone of 1.5 x the cutoff angle about the spot's axis (plateau, band and
    dark region all drawn), 0.5 .. 4 away from the light."""
    sp = SPOTS[k]
    rng = np.random.default_rng(seed + k)
    pos = sp["pos"].astype(np.float64)
    axis = sp["target"].astype(np.float64) - pos
    axis /= np.linalg.norm(axis)
    a = np.array([1.0, 0, 0]) if abs(axis[0]) < 0.9 else np.array([0, 1.0, 0])
    u = np.cross(axis, a)
    u /= np.linalg.norm(u)
    v = np.cross(axis, u)
    m = 6 * n
    theta = np.radians(min(1.5 * float(sp["cutoff"]), 170.0)) * rng.random(m)
    phi = 2 * np.pi * rng.random(m)
    dist = 0.5 + 3.5 * rng.random(m)
    dirs = np.cos(theta)[:, None] * axis + np.sin(theta)[:, None] * (np.cos(phi)[:, None] * u + np.sin(phi)[:, None] * v)
    ref = f32(pos + dirs * dist[:, None]).astype(np.float64)
    keep = _well_conditioned(np.broadcast_to(pos, ref.shape), ref)
    assert keep.sum() >= n
    return f32(ref[keep][:n])


def distant_refs(n=4096, seed=7):
    """Points of a ball of radius 4; those in front of the disk keep the conditioning rule with
    p = ref - distance d, those behind it (value 0) are all kept."""
    rng = np.random.default_rng(seed)
    ref = f32(_ball(rng, 8 * n, 4.0)).astype(np.float64)
    r = LR.distant(DISTANT["E"], DISTANT["dir"], DISTANT["r"], ref)
    keep = ~r["lit"] | _well_conditioned(r["p"], ref)
    front = np.nonzero(keep & r["lit"])[0][:n // 2]
    back = np.nonzero(keep & ~r["lit"])[0][:n - front.size]
    assert front.size + back.size == n and front.size >= n // 4
    return f32(ref[np.sort(np.concatenate([front, back]))])


def random_sets(ctl):
    """[(name, queries, float64 reference dict)] of the evaluator scene, 4096 queries each."""
    out = [("point", queries(ctl, I_POINT, point_refs()), None)]
    out[0] = (out[0][0], out[0][1], LR.point(POINT["pos"], POINT["I"], out[0][1]["ref"]))
    for k, sp in enumerate(SPOTS):
        q = queries(ctl, I_SPOT0 + k, spot_refs(k))
        out.append((f"spot{k}", q, LR.spot(sp["pos"], sp["target"], sp["I"], sp["cutoff"], sp["beam"], q["ref"])))
    q = queries(ctl, I_DISTANT, distant_refs())
    out.append(("distant", q, LR.distant(DISTANT["E"], DISTANT["dir"], DISTANT["r"], q["ref"])))
    return out


# ---------------------------------------------------------------------------------------------
# Edge queries: a scene of its own whose lights sit on the axes, so that fp32 arithmetic can be
# followed by hand.
EDGE_SPOT = dict(pos=f32([0, 0, 0]), target=f32([0, 0, 1]), I=f32([2.0, 3.0, 4.0]), cutoff=F(50.0), beam=F(35.0))
EDGE_EQ = [dict(pos=f32([0, 0, 0]), target=f32([0, 0, 1]), I=f32([1.0, 2.0, 3.0]), cutoff=F(90.0), beam=F(90.0)),
           dict(pos=f32([0, 0, 0]), target=f32([0, 0, 1]), I=f32([1.0, 2.0, 3.0]), cutoff=F(30.0), beam=F(30.0))]
EDGE_DISTANT = dict(E=f32([0.5, 0.25, 2.0]), dir=f32([0, 0, 1]), r=F(1.0))
EDGE_POINT = dict(pos=f32([0.5, -0.25, 2.0]), I=f32([1.0, 1.0, 1.0]))
E_SPOT, E_EQ0, E_DISTANT, E_POINT = 0, 1, 3, 4


@functools.lru_cache(maxsize=None)
def edge_scene(ctl):
    s = ctl.HostScene()
    m = Mesh()
    floor_mesh(m)
    s.add_node(m.add_to(s, [ctl.diffuse_material(*RHO)]))
    s.set_camera((0, 0, 4), (0, 0, 0), (0, 1, 0), 40.0, 64, 64)
    for sp in [EDGE_SPOT] + EDGE_EQ:
        s.add_spot_light(sp["pos"], sp["target"], sp["I"], sp["cutoff"], sp["beam"])
    s.add_distant_light(EDGE_DISTANT["E"], EDGE_DISTANT["dir"], EDGE_DISTANT["r"])
    s.add_point_light(EDGE_POINT["pos"], EDGE_POINT["I"])
    return s, s.compile()


def light_slot(desc, i):
    """The ctl_light_params slot of delta light i."""
    import cudatracerlib_amd._abi as A
    L = desc.lights[i]
    assert L.tri_count == 0 and L.tri_first < desc.n_light_tris
    return A.LightParams.from_buffer_copy(desc.light_tris[L.tri_first])


def _axis_cos(x):
    """cosTheta of the spot at the origin looking along +z for ref = (x, 0, 1), as fp32 computes it:
    dir = pos - ref = (-x, -0, -1); dist = sqrt((x*x + 0) + 1); invDist = 1 / dist; -d.z = 1 * invDist."""
    x = f32(x)
    dist = np.sqrt((F(0) + x * x + F(0)) + F(1), dtype=np.float32)
    return F(1) / dist


def refs_with_cos_theta(c, lo=0.0, hi=8.0):
    """fp32 x with _axis_cos(x) == c exactly (c an fp32 cosine in (0.13, 1)): bisection to the
    neighbourhood, then the adjacent floats."""
    c = F(c)
    a, b = F(lo), F(hi)
    for _ in range(60):
        mid = F((a + b) / 2)
        if _axis_cos(mid) > c:
            a = mid
        else:
            b = mid
    xs = [a]
    for _ in range(64):
        xs.append(np.nextafter(xs[-1], F(-1)))
    x = xs[0]
    for _ in range(64):
        x = np.nextafter(x, F(100))
        xs.append(x)
    xs = f32(xs)
    return xs[_axis_cos(xs) == c]


def edge_sets(ctl):
    """{name: queries} of the edge scene.  Expectations are in test_lights_host.py."""
    _, d = edge_scene(ctl)
    P = light_slot(d, E_SPOT)
    out = {}
    for name, c in (("cutoff", P.cos_cutoff_angle), ("beam", P.cos_beam_width)):
        xs = refs_with_cos_theta(c)
        assert xs.size >= 1, name
        out["spot_at_" + name] = queries(ctl, E_SPOT, np.stack([xs, np.zeros_like(xs), np.ones_like(xs)], 1))
    radius = F(EDGE_DISTANT["r"]) * F(1.1)
    out["distant_on_plane"] = queries(ctl, E_DISTANT, [[0.25, -0.5, radius], [3.0, 2.0, radius]])
    out["distant_behind"] = queries(ctl, E_DISTANT, [[0.25, -0.5, np.nextafter(radius, F(0))], [0.0, 0.0, 0.0],
                                                     [1.0, 1.0, -5.0]])
    rng = np.random.default_rng(3)
    ref = f32(_ball(rng, 512, 3.0))
    ref = ref[np.linalg.norm(ref, axis=1) > 0.25]
    for k in range(2):
        out[f"equal_angles{k}"] = queries(ctl, E_EQ0 + k, ref)
    out["ref_is_pos"] = np.concatenate([queries(ctl, E_POINT, [EDGE_POINT["pos"]]), queries(ctl, E_SPOT, [EDGE_SPOT["pos"]]),
                                        queries(ctl, E_EQ0, [EDGE_SPOT["pos"]])])
    return out


# ---------------------------------------------------------------------------------------------
# The mixed scene: an area light, the environment and one light of each new kind, on one instance
# or on two (the second mesh under its own node, so the non-SINGLE kernels run).
def _sky(ctl, s):
    rng = np.random.default_rng(5)
    yy = np.arange(8)[:, None]
    img = ((40 + 20 * yy + rng.integers(0, 30, size=(8, 16))).astype(np.uint32) * 0x010101) | 0xff000000
    return s.add_texture(img.astype(np.uint32), filter=ctl._abi.CTL_TEX_BILINEAR)


MIXED_POINT = dict(pos=f32([-1.5, 1.75, -1.0]), I=f32([4.0, 3.5, 3.0]))
MIXED_SPOT = dict(pos=f32([1.5, 2.5, -1.5]), target=f32([0.5, 0.0, 0.0]), I=f32([9.0, 8.0, 6.0]), cutoff=F(35.0), beam=F(20.0))
# the distant lights of the rendered scenes travel downwards; their negative scene radius puts the
# disk's plane (dot(ref, dir) = 1.1 r, the reference's rule) above the whole scene, so all of it is lit
MIXED_DISTANT = dict(E=f32([0.75, 0.75, 1.0]), dir=f32([1.0, -3.0, 1.0]), r=F(-9.0))


def add_mixed_delta_lights(s, point=MIXED_POINT):
    return [s.add_point_light(point["pos"], point["I"]),
            s.add_spot_light(MIXED_SPOT["pos"], MIXED_SPOT["target"], MIXED_SPOT["I"], MIXED_SPOT["cutoff"], MIXED_SPOT["beam"]),
            s.add_distant_light(MIXED_DISTANT["E"], MIXED_DISTANT["dir"], MIXED_DISTANT["r"])]


def mixed_host_scene(ctl, w=64, h=64, instances=1, delta=True, point=MIXED_POINT):
    """A textured diffuse floor, a small area light, the environment, a rough conductor card; with
    instances = 2 the card is a mesh of its own under a second, moved node."""
    import bsdf_cases as BC
    s = ctl.HostScene()
    sky = _sky(ctl, s)
    rng = np.random.default_rng(11)
    tex = s.add_texture((rng.integers(60, 250, size=(8, 8)).astype(np.uint32) * 0x010101 | 0xff000000).astype(np.uint32),
                        filter=ctl._abi.CTL_TEX_BILINEAR)
    card = ctl.roughconductor_material(1, BC.GOLD_ETA, BC.GOLD_K, 0.25)
    mats = [ctl.diffuse_material(0.6, 0.6, 0.55, texture=tex), ctl.diffuse_material(0.8, 0.8, 0.8)]
    m = Mesh()
    m.quad([(-6, 0, -6), (-6, 0, 6), (6, 0, 6), (6, 0, -6)], 0)
    m.quad([(-0.4, 3.0, -0.4), (0.4, 3.0, -0.4), (0.4, 3.0, 0.4), (-0.4, 3.0, 0.4)], 1)   # light, facing down
    cardq = [(-0.9, 0.05, 0.6), (-0.9, 1.4, 1.2), (0.9, 1.4, 1.2), (0.9, 0.05, 0.6)]         # faces the camera
    if instances == 1:
        m.quad(cardq, 2)
        node = s.add_node(m.add_to(s, mats + [card]))
    else:
        node = s.add_node(m.add_to(s, mats))
        m2 = Mesh()
        m2.quad(cardq, 0)
        s.add_node(m2.add_to(s, [card]), [1, 0, 0, 0.5, 0, 1, 0, 0.0, 0, 0, 1, 0.25, 0, 0, 0, 1])
    s.add_area_light(node, 1, (14.0, 14.0, 14.0))
    s.set_environment(sky, (0.5, 0.45, 0.4))
    s.set_camera((0.3, 2.0, -5.5), (0.0, 0.6, 0.0), (0, 1, 0), 50.0, w, h)
    lights = add_mixed_delta_lights(s, point) if delta else []
    return s, lights


def desc_bytes(ctl, d):
    """Every array and every scalar field of a scene description as bytes, by field name."""
    from cudatracerlib_amd import scene_cache
    out = {}
    for name, (et, count) in scene_cache._ARRAYS.items():
        addr = C.cast(getattr(d, name), C.c_void_p).value
        n = int(count(d)) if addr else 0
        if name == "env" and d.env_map_index == 0xFFFFFFFF:
            n = 0
        out[name] = C.string_at(addr, n * C.sizeof(et)) if n else b""
    for name, _ in type(d)._fields_:
        if name not in scene_cache._ARRAYS:
            f = getattr(type(d), name)
            out[name] = bytes(d)[f.offset:f.offset + f.size]
    return out


# ---------------------------------------------------------------------------------------------
# Analytic renders: the floor z = 0 under one light, camera straight above (every view ray within
# 30 degrees of the normal), every light direction within 60 degrees of it.
CAM = dict(pos=(0.0, 0.0, 4.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov=40.0)
A_POINT = dict(pos=f32([0.5, -0.25, 2.0]), I=f32([3.0, 2.5, 2.0]))
# axis 30 degrees off the normal; at the floor the plateau, the band and the dark region each cover > 10 %
A_SPOT = dict(pos=f32([-0.5, 0.0, 2.0]), target=f32([0.25, 0.25, 0.0]), I=f32([6.0, 5.0, 4.0]), cutoff=F(32.0), beam=F(16.0))
A_DISTANT = dict(E=f32([1.25, 1.0, 0.75]), dir=f32([1.0, 0.5, -2.0]), r=F(-5.0))
ANALYTIC = {"point": A_POINT, "spot": A_SPOT, "distant": A_DISTANT}


def add_analytic_light(s, kind, L=None, scale=1.0):
    L = ANALYTIC[kind] if L is None else L
    if kind == "point":
        return s.add_point_light(L["pos"], L["I"] * F(scale))
    if kind == "spot":
        return s.add_spot_light(L["pos"], L["target"], L["I"] * F(scale), L["cutoff"], L["beam"])
    return s.add_distant_light(L["E"] * F(scale), L["dir"], L["r"])


# The shadow scenes: a quad parallel to the floor (x and y ranges), beside the camera's view (at
# z = 0.75 the view ends at |x| = 1.19), lit from further out so that its shadow falls into the view.
OCCLUDER = dict(z=0.75, lo=(1.5, -1.0), hi=(2.75, 1.0))
S_POINT = dict(pos=f32([3.75, 0.0, 1.5]), I=f32([3.0, 2.5, 2.0]))
S_DISTANT = dict(E=f32([1.25, 1.0, 0.75]), dir=f32([-1.5, 0.0, -1.0]), r=F(-5.0))
SHADOW = {"point": S_POINT, "distant": S_DISTANT}


def analytic_scene(ctl, kind, w=64, h=64, occluder=False, copies=1, L=None):
    """The floor, optionally the occluder quad above it, and `copies` co-located lights of `kind`
    (ANALYTIC[kind], or L) sharing the intensity."""
    s = ctl.HostScene()
    m = Mesh()
    floor_mesh(m)
    if occluder:
        (x0, y0), (x1, y1), z = OCCLUDER["lo"], OCCLUDER["hi"], OCCLUDER["z"]
        m.quad([(x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)], 0)
    s.add_node(m.add_to(s, [ctl.diffuse_material(*RHO)]))
    s.set_camera(CAM["pos"], CAM["target"], CAM["up"], CAM["fov"], w, h)
    for _ in range(copies):
        add_analytic_light(s, kind, L=L, scale=1.0 / copies)
    return s, s.compile()


def floor_normals_exact(ctl, d):
    """The floor's three vertex normals decode from their 16-bit codes to (0, 0, 1) exactly."""
    for t in range(2):
        w = d.tri_data[t].w
        codes = np.array([w[0] & 0xffff, w[0] >> 16, w[1] & 0xffff], np.uint32)
        n = ctl.host_math_eval("normal_decode16", codes).view(np.float32).reshape(3, 3)
        if not np.array_equal(n, np.tile(f32([0, 0, 1]), (3, 1))):
            return False
    return True


def pixel_corner_rays(d, px, py):
    """Float64 camera rays through sample positions (px, py) (pixel units): origin, unit directions."""
    cam = d.camera
    tw = np.array(cam.to_world.m[:], np.float64).reshape(4, 4)
    s2c = np.array(cam.sample_to_camera.m[:], np.float64).reshape(4, 4)
    ir = np.array(cam.inv_resolution[:], np.float64)
    p = np.stack([px * ir[0], py * ir[1], np.zeros_like(px), np.ones_like(px)], 1) @ s2c.T
    p = p[:, :3] / p[:, 3:4]
    dd = p / np.linalg.norm(p, axis=1, keepdims=True)
    return tw[:3, 3], dd @ tw[:3, :3].T


def back_project(d, dirs):
    """Sample positions (pixel units) of float64 world directions from the camera: the inverse of
    pixel_corner_rays."""
    cam = d.camera
    tw = np.array(cam.to_world.m[:], np.float64).reshape(4, 4)
    s2c = np.array(cam.sample_to_camera.m[:], np.float64).reshape(4, 4)
    ir = np.array(cam.inv_resolution[:], np.float64)
    local = np.asarray(dirs, np.float64) @ tw[:3, :3]          # inverse rotation (orthonormal)
    # nearP = s2c (sx, sy, 0, 1) is affine in (sx, sy): solve for the point of the near plane on the ray
    o = s2c @ np.array([0, 0, 0, 1.0])
    ex = s2c @ np.array([1.0, 0, 0, 1.0])
    ey = s2c @ np.array([0, 1.0, 0, 1.0])
    assert o[3] == ex[3] == ey[3]
    o, ex, ey = o[:3] / o[3], ex[:3] / ex[3], ey[:3] / ey[3]
    near = local * (o[2] / local[:, 2])[:, None]
    sx = (near[:, 0] - o[0]) / (ex[0] - o[0])
    sy = (near[:, 1] - o[1]) / (ey[1] - o[1])
    return sx / ir[0], sy / ir[1]


def floor_points(origin, dirs):
    t = -origin[2] / dirs[:, 2]
    return origin[None, :] + t[:, None] * dirs


def irradiance(kind, P, L=None):
    """Float64 (E (n, 3), cos_theta, extras) at floor points P (normal +z): E is the irradiance term
    of the issue (I / d^2, I falloff / d^2, or the distant E), cos_theta the light's incidence cosine."""
    L = ANALYTIC[kind] if L is None else L
    if kind == "point":
        r = LR.point(L["pos"], L["I"], P)
    elif kind == "spot":
        r = LR.spot(L["pos"], L["target"], L["I"], L["cutoff"], L["beam"], P)
    else:
        r = LR.distant(L["E"], L["dir"], L["r"], P)
    return r["value"], r["d"][:, 2], r


def occluded(kind, P, margin):
    """Per floor point: +1 when the float64 shadow ray (towards SHADOW[kind]) passes through the
    occluder's interior more than `margin` x its shorter edge from the border, -1 when it misses the
    quad by more than that, else 0."""
    _, _, r = irradiance(kind, P, SHADOW[kind])
    d = r["d"]
    t = (OCCLUDER["z"] - P[:, 2]) / d[:, 2]
    x, y = P[:, 0] + t * d[:, 0], P[:, 1] + t * d[:, 1]
    (x0, y0), (x1, y1) = OCCLUDER["lo"], OCCLUDER["hi"]
    m = margin * min(x1 - x0, y1 - y0)
    inside = np.minimum(np.minimum(x - x0, x1 - x), np.minimum(y - y0, y1 - y))   # > 0 inside, distance to the border
    below_light = t < r["dist"]
    return np.where((inside > m) & below_light, 1, np.where((inside < -m) | ~below_light, -1, 0))
