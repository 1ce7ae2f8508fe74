"""Scenes and framebuffer checks for the material tests, shared by the GPU tests
(test_gpu_materials.py, test_gpu_materials_oracle.py) and the oracle's own (test_oracle_materials.py).

Scene A (mixed_scene): one mesh under one node, one card per type, an area light, an environment
map: the single-instance kernels and every BSDF's ordinary branches.
Scene B (events_scene): two meshes under two nodes for what A does not reach: the inside of a glass
cube (wi.z < 0, the inverse eta, total internal reflection, paths cut by max_path_length), ext
records behind a material_offset > 0, a transformed node, an emitter and the environment seen
through specular bounces, NEE on a material with a delta and a smooth lobe, anisotropic rough
conductors and a textured non-linear plastic.

The three closed-form checks take a framebuffer, so they judge the oracle's image as they judge the
device's."""
import ctypes as C
import functools

import numpy as np

import bsdf_cases as BC
import bsdf_ref as R
import oracle
from helpers import jitter_landing, select_bvh, tie_rule

U = 2.0 ** -24
ENV_RGB = (200, 180, 160)


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

    def box(self, lo, hi, k):
        """A closed box, 12 triangles, faces wound to look outwards."""
        (x0, y0, z0), (x1, y1, z1) = lo, hi
        self.quad([(x0, y0, z0), (x0, y1, z0), (x1, y1, z0), (x1, y0, z0)], k)   # -z
        self.quad([(x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)], k)   # +z
        self.quad([(x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0)], k)   # -x
        self.quad([(x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1)], k)   # +x
        self.quad([(x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1)], k)   # -y
        self.quad([(x0, y1, z0), (x0, y1, z1), (x1, y1, z1), (x1, y1, z0)], k)   # +y

    def add_to(self, s, mats):
        return s.add_mesh(np.array(self.v, np.float32), np.array(self.i, np.uint32), mats,
                          mat_index=np.array(self.m, np.uint8), uvs=np.array(self.uv, np.float32))


def same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def first_differences(got, want, w):
    """The first differing pixels of two framebuffers, for an assertion message."""
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))[0]
    return (f"{bad.size} of {got.shape[0]} pixels differ; first: "
            + "; ".join(f"({int(i) % w}, {int(i) // w}) got {got[i].tolist()} want {want[i].tolist()}" for i in bad[:3]))


def _sky(ctl, s, seed):
    rng = np.random.default_rng(seed)
    yy = np.arange(8)[:, None]
    img = ((40 + 20 * yy + rng.integers(0, 30, size=(8, 16))).astype(np.uint32) * 0x010101) | 0xff000000
    s.set_environment(s.add_texture(img.astype(np.uint32), filter=ctl._abi.CTL_TEX_BILINEAR), (1.5, 1.4, 1.3))


def mixed_scene(ctl, w=48, h=48):
    """Scene A: a diffuse floor, an area light, the environment, and one tilted card per new type."""
    s = ctl.HostScene()
    _sky(ctl, s, 5)
    gold = (BC.GOLD_ETA, BC.GOLD_K)
    mats = [ctl.diffuse_material(0.6, 0.6, 0.55), ctl.diffuse_material(0.8, 0.8, 0.8),
            ctl.dielectric_material(1.5), ctl.thindielectric_material(1.5, (0.9, 0.9, 1.0), (0.9, 1.0, 0.9)),
            ctl.conductor_material(*gold, (0.95, 0.9, 0.85)), ctl.roughconductor_material(1, *gold, 0.2),
            ctl.plastic_material(1.5, (0.2, 0.4, 0.7), nonlinear=True)]
    m = Mesh()
    m.quad([(-6, 0, -6), (-6, 0, 6), (6, 0, 6), (6, 0, -6)], 0)
    m.quad([(-0.8, 3.0, -0.8), (0.8, 3.0, -0.8), (0.8, 3.0, 0.8), (-0.8, 3.0, 0.8)], 1)   # light, facing down
    # cards leaning back; their winding turns the normal cross(v1 - v0, v2 - v0) away from the camera, so
    # it sees the back of the one-sided types (conductor, rough conductor, plastic: black from there) and
    # the glass from inside.  Scene B's cards face the camera.
    for k in range(5):
        x = -2.6 + 1.3 * k
        m.quad([(x - 0.55, 0.05, -0.3), (x + 0.55, 0.05, -0.3), (x + 0.55, 1.3, 0.5), (x - 0.55, 1.3, 0.5)], 2 + k)
    node = s.add_node(m.add_to(s, mats))
    s.add_area_light(node, 1, (14.0, 14.0, 14.0))
    s.set_camera((0.3, 2.0, -5.5), (0.0, 0.6, 0.0), (0, 1, 0), 50.0, w, h)
    return s, s.compile()


def _rot_y(angle, trans):
    """Row-major float4x4: a rotation about y, then a translation (in the last column)."""
    c, s = np.cos(angle), np.sin(angle)
    return [c, 0, s, trans[0], 0, 1, 0, trans[1], -s, 0, c, trans[2], 0, 0, 0, 1]


def events_scene(ctl, w=48, h=48):
    """Scene B.  Mesh 0 under node 0 (materials without ext records): a diffuse floor, the area light
    and a closed glass box, 12 triangles (eta 1.5, one-sided, R != T != 1).  Mesh 1 under node 1, which is turned
    about y and moved, so its material_offset is 3 and its ext records follow mesh 0's: a conductor
    card leaning so that the camera sees the light in it, a non-linear plastic card whose diffuse
    reflectance is a bilinear image texture, an anisotropic GGX and a Beckmann rough conductor card,
    and a two-sided thindielectric pane in front of part of the floor."""
    s = ctl.HostScene()
    _sky(ctl, s, 9)
    rng = np.random.default_rng(11)
    tex_img = (rng.integers(40, 230, size=(8, 8)).astype(np.uint32) | (rng.integers(40, 230, size=(8, 8)).astype(np.uint32) << 8)
               | (rng.integers(40, 230, size=(8, 8)).astype(np.uint32) << 16) | 0xff000000)
    tex = s.add_texture(tex_img.astype(np.uint32), filter=ctl._abi.CTL_TEX_BILINEAR)
    avg = [float(((tex_img >> (8 * c)) & 0xff).mean() / 255.0) for c in range(3)]
    m0 = Mesh()
    m0.quad([(-6, 0, -6), (-6, 0, 6), (6, 0, 6), (6, 0, -6)], 0)
    m0.quad([(-1.2, 3.2, -1.2), (1.2, 3.2, -1.2), (1.2, 3.2, 1.2), (-1.2, 3.2, 1.2)], 1)   # light, facing down
    m0.box((-3.0, 0.005, -3.0), (-0.8, 2.0, -1.0), 2)
    mesh0 = m0.add_to(s, [ctl.diffuse_material(0.6, 0.6, 0.55), ctl.diffuse_material(0.8, 0.8, 0.8),
                          ctl.dielectric_material(1.5, (0.9, 0.85, 0.8), (0.8, 0.9, 0.95))])
    m1 = Mesh()
    # in the node's frame: the cards stand on z = 0 leaning back (towards +z); their winding makes the
    # normal cross(v1 - v0, v2 - v0) point to -z and up, at the camera (these BSDFs are one-sided)
    m1.quad([(-0.4, 0.05, 0.0), (-0.4, 1.1, 1.05), (0.6, 1.1, 1.05), (0.6, 0.05, 0.0)], 0)   # conductor, 45 degrees
    m1.quad([(-2.6, 0.05, 0.0), (-2.6, 1.3, 0.6), (-1.6, 1.3, 0.6), (-1.6, 0.05, 0.0)], 1)   # plastic
    m1.quad([(-1.5, 0.05, 0.0), (-1.5, 1.3, 0.6), (-0.5, 1.3, 0.6), (-0.5, 0.05, 0.0)], 2)   # GGX rough conductor
    m1.quad([(0.7, 0.05, 0.0), (0.7, 1.3, 0.6), (1.7, 1.3, 0.6), (1.7, 0.05, 0.0)], 3)       # Beckmann rough conductor
    m1.quad([(0.2, 0.1, -1.6), (1.8, 0.1, -1.6), (1.8, 1.0, -1.5), (0.2, 1.0, -1.5)], 4)     # pane before the floor
    mesh1 = m1.add_to(s, [ctl.conductor_material(BC.GOLD_ETA, BC.GOLD_K, (0.95, 0.9, 0.85)),
                          ctl.plastic_material(1.5, (0.5, 0.5, 0.5), (1.0, 0.9, 0.8), nonlinear=True, texture=tex,
                                               diffuse_average=avg),
                          ctl.roughconductor_material(1, BC.ALU_ETA, BC.ALU_K, 0.12, 0.3),
                          ctl.roughconductor_material(0, BC.GOLD_ETA, BC.GOLD_K, 0.25),
                          ctl.thindielectric_material(1.5, (0.9, 0.9, 1.0), (0.9, 1.0, 0.9), two_sided=True)])
    n0 = s.add_node(mesh0)
    s.add_node(mesh1, _rot_y(0.2, (0.9, 0.0, 0.6)))
    s.add_area_light(n0, 1, (14.0, 14.0, 14.0))
    s.set_camera((0.2, 2.2, -6.0), (0.0, 0.6, 0.0), (0, 1, 0), 50.0, w, h)
    d = s.compile()
    assert d.n_nodes == 2 and d.nodes[1].material_offset == 3 and d.materials_ext
    return s, d


SCENES = {"A": mixed_scene, "B": events_scene}
W = H = 48
# the renders the tests make of a scene: name -> (max_path_length, rr_start_depth, passes).  "long" is
# scene B's second render: Russian roulette from the second hit on, paths cut inside the glass at 50.
RENDERS = {"std": (12, 3, 3), "long": (50, 1, 3)}
# what each render of each scene must reach at least EVENT_FLOOR times (tests/test_oracle_materials.py
# checks it on the oracle's counters).  nee_on_delta_and_smooth exists only with Direct = 1: without
# it the integrator makes no next-event estimate at all.
EVENT_FLOOR = 50
EVENTS_OF = {("A", "std"): ("delta_bounce", "env_after_specular", "nee_on_delta_and_smooth", "rr_draw"),
             ("B", "std"): ("tir", "emitter_after_specular", "env_after_specular", "nee_on_delta_and_smooth",
                            "ended_by_length", "rr_draw", "delta_bounce"),
             ("B", "long"): ("tir", "emitter_after_specular", "env_after_specular", "nee_on_delta_and_smooth",
                             "ended_by_length", "rr_draw", "delta_bounce")}


@functools.lru_cache(maxsize=None)
def scene(name, w=W, h=H):
    """(host scene, desc) of scene A or B, built once per process."""
    import cudatracerlib_amd as ctl
    return SCENES[name](ctl, w, h)


def pt_params(ctl, direct, render="std", flags=0, num_ranks=1, rank=0, tile=16):
    mpl, rr, _ = RENDERS[render]
    return ctl.PTParams(direct, mpl, rr, 1, tile, num_ranks, rank, flags)


@functools.lru_cache(maxsize=None)
def reference(name, direct, bvh="wide", render="std"):
    """The oracle's render of a scene, computed once and shared (do not write to it):
    (framebuffer, rays, event counts summed over the passes)."""
    import cudatracerlib_amd as ctl
    orc = oracle.load()
    d = select_bvh(scene(name)[1], bvh)
    p = pt_params(ctl, direct, render)
    fb = np.zeros((W * H, 7), np.float32)
    rays, events = 0, dict.fromkeys(oracle.EVENTS, 0)
    for k in range(RENDERS[render][2]):
        r, ev = oracle.render_pass_events(d, p, k, fb, tie_rule(d, orc))
        rays += r
        for name_, n in ev.items():
            events[name_] += n
    fb.setflags(write=False)
    return fb, rays, events


# ---------------------------------------------------------------------------------------------
# the three closed-form renders
def env_only(ctl, w, h, cam):
    s = ctl.HostScene()
    uniform_env(s, ctl)
    s.set_camera(*cam, w, h)
    return s, s.compile()


PANES_CAM = ((0.0, 0.2, 5.0), (0.0, 0.0, 0.0), (0, 1, 0), 40.0)


def invisible_panes_scene(ctl, w, h):
    """thindielectric panes with reflectance = transmittance = 1 under a one-colour environment and
    nothing else: (scene, desc)."""
    s = ctl.HostScene()
    uniform_env(s, ctl)
    m = Mesh()
    for k, z in enumerate((0.0, 0.7, 1.5, 2.2)):   # overlapping in depth, of different sizes, one tilted
        e = 3.0 - 0.6 * k
        t = 0.4 if k == 2 else 0.0
        m.quad([(-e, -e, z - t), (e, -e, z - t), (e, e, z + t), (-e, e, z + t)], 0)
    s.add_node(m.add_to(s, [ctl.thindielectric_material(1.5, (1.0, 1.0, 1.0), (1.0, 1.0, 1.0))]))
    s.set_camera(*PANES_CAM, w, h)
    return s, s.compile()


def check_invisible_panes(got, want, passes, label):
    """got: the render with the panes; want: the oracle's render of the environment alone.  Every
    event multiplies the throughput by exactly 1, a delta bounce skips Russian roulette, and the
    escaped path's MIS weight is 1 after a specular bounce, so each sample adds
    1 * EvalEnvironment(last ray).

    Bound: the bilinear lookup of a constant c is a sum of four terms (1-ds)(1-dt) c, each with at
    most 4 roundings (two differences, two products), summed with 3 additions: within 7 * 2^-24 of c;
    the scale product 1 more; the framebuffer's 4 samples are summed with 3 additions: 11 * 2^-24.
    The render with the panes looks the constant up in other directions than the render without, so
    the two differ by at most 22 * 2^-24 relative."""
    assert np.array_equal(got[:, 6], want[:, 6]) and want[:, 6].max() >= passes - 1
    lit = want[:, 6] > 0
    rel = np.abs(got[lit, :3].astype(np.float64) / want[lit, :3].astype(np.float64) - 1.0)
    print(f"invisible panes, {label}: worst {rel.max() / U:.2f} roundings")
    assert rel.max() <= 22 * U


MIRROR_CAM = ((0.3, 0.2, 4.0), (0.0, 0.0, 0.0), (0, 1, 0), 35.0)
MIRROR_REFL = (0.9, 0.75, 0.6)


def _half(h16):
    return np.array([h16], np.uint16).view(np.float16).astype(np.float32)[0]


def mirror_wall_scene(ctl, w, h):
    """One conductor quad in the plane z = 0 filling the view, facing +z: (scene, desc)."""
    s = ctl.HostScene()
    uniform_env(s, ctl)
    m = Mesh()
    m.quad([(-4, -4, 0), (4, -4, 0), (4, 4, 0), (-4, 4, 0)], 0)
    s.add_node(m.add_to(s, [ctl.conductor_material(BC.GOLD_ETA, BC.GOLD_K, MIRROR_REFL)]))
    s.set_camera(*MIRROR_CAM, w, h)
    d = s.compile()
    # the compiled TriangleData: all six vertex normals carry code 0, dpdu and dpdv are axis vectors
    for t in range(2):
        wds = d.tri_data[t].w
        assert wds[0] == 0 and (wds[1] & 0xffff) == 0
        dpdu = [_half(wds[2] & 0xffff), _half(wds[2] >> 16), _half(wds[3] & 0xffff)]
        dpdv = [_half(wds[3] >> 16), _half(wds[4] & 0xffff), _half(wds[4] >> 16)]
        assert dpdu[1] == 0 and dpdu[2] == 0 and dpdu[0] > 0 and dpdv[0] == 0 and dpdv[2] == 0 and dpdv[1] > 0, (dpdu, dpdv)
    return s, d


def check_mirror_wall(orc, got, env, d, w, h):
    """got: one pass of the mirror scene with max_path_length 2, Direct 0; env: the oracle's pass of the
    environment alone.  A pixel's sample is reflectance * fresnelConductorExact(wi.z) *
    EvalEnvironment(reflected ray), wi.z = dot(-d, sys.n) with sys.n = (0, 0, nz).  nz comes out of
    three normalisations x * (1 / x) of vectors along one axis; such a product is 1 or 1 - 2^-24,
    never more, so wi.z is -d.z or its neighbour below, and either is accepted.  The environment
    factor lies in the value range of the render without the quad (the constant map, up to the
    lookup's rounding), and the fp32 product may be one ulp off either end of that range."""
    lo, hi = env[env[:, 6] > 0, :3].min(axis=0), env[:, :3].max(axis=0)
    # the constant map, up to the bilinear lookup's rounding: 8 roundings either way (check_invisible_panes)
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
            f = np.array([np.float32(MIRROR_REFL[c]) * F[c] for c in range(3)], np.float32)
            ok = ok or ((px >= np.nextafter(f * lo, -inf)).all() and (px <= np.nextafter(f * hi, inf)).all())
        assert ok, (i, px, f * lo, f * hi)
        checked += 1
    assert checked > 0.9 * w * h


def textured_plastic_scene(ctl, nonlinear, textured, w=32, h=32):
    """A plastic floor under an area light; m_diffuseReflectance is an image texture of one colour
    (point-sampled: the texel is the colour itself) or the constant of that colour (the texel 80 / 255
    decodes to the same float the constant is given as)."""
    c = np.float32(80) / np.float32(255)
    s = ctl.HostScene()
    tex = s.add_texture(np.full((8, 8), 0xff505050, np.uint32), filter=ctl._abi.CTL_TEX_POINT)
    pl = ctl.plastic_material(1.5, (c, c, c), nonlinear=nonlinear, texture=tex if textured else None)
    m = Mesh()
    m.quad([(-3, 0, -3), (-3, 0, 3), (3, 0, 3), (3, 0, -3)], 0)
    m.quad([(-0.5, 2.0, -0.5), (0.5, 2.0, -0.5), (0.5, 2.0, 0.5), (-0.5, 2.0, 0.5)], 1)
    node = s.add_node(m.add_to(s, [pl, ctl.diffuse_material(0.8, 0.8, 0.8)]))
    s.add_area_light(node, 1, (10.0, 10.0, 10.0))
    s.set_camera((0.2, 1.5, -4.0), (0.0, 0.0, 0.0), (0, 1, 0), 50.0, w, h)
    d = s.compile()
    assert d.materials[0].texture == (0 if textured else 0xFFFFFFFF)
    return s, d


def check_textured_plastic(a, b):
    """a: the render with the one-colour texture; b: with the constant.  Bit equality."""
    assert same(a, b), first_differences(a, b, 32)
    assert a[:, :3].max() > 0 and np.isfinite(a).all()
