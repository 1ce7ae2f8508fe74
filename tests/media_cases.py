"""Volumes, scenes and query sets of the participating-media tests, shared by test_media_host.py (CPU)
and test_gpu_media.py.  Every number that reaches the library is fp32-representable, so the float64
reference (media_ref.py) and the library start from the same inputs."""
import functools

import numpy as np

import media_ref as MR
from light_cases import floor_mesh, RHO
from materials_scenes import Mesh

F = np.float32
FLT_MAX = np.finfo(np.float32).max
N_RANDOM = 4096
OPS = ("intersect", "transmittance", "sample_distance", "phase_eval", "phase_sample")


def f32(a):
    return np.asarray(a, np.float32)


def trs(scale, translate, rot_deg=(0.0, 0.0, 0.0)):
    """translate * Rz * Ry * Rx * scale as a row-major 4x4, rounded to fp32."""
    rx, ry, rz = np.radians(rot_deg)
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    M = np.eye(4)
    M[:3, :3] = Rz @ Ry @ Rx @ np.diag(np.asarray(scale, np.float64))
    M[:3, 3] = translate
    return M.astype(np.float32)


# The axis-aligned box [-2, 2]^3 and a rotated, non-uniformly scaled one (edges 3, 5 and 4 long).
AXIS_BOX = trs((4.0, 4.0, 4.0), (-2.0, -2.0, -2.0))
TILTED_BOX = trs((3.0, 5.0, 4.0), (-1.25, -2.5, -1.5), (20.0, -35.0, 50.0))


def volume(to_world, sig_a, sig_s, phase="isotropic", g=0.0):
    to_world = f32(to_world)
    return dict(to_world=to_world, w2v=np.linalg.inv(to_world.astype(np.float64)), sig_a=f32(sig_a), sig_s=f32(sig_s),
                phase=phase, g=float(F(g)))


G_VALUES = (0.0, 1e-9, 0.3, -0.3, 0.9, -0.9)
VOLUMES = {
    "tilted_hg": volume(TILTED_BOX, (0.125, 0.25, 0.5), (0.5, 0.75, 0.25), "hg", 0.3),
    "axis_iso": volume(AXIS_BOX, (0.25, 0.25, 0.25), (0.75, 0.75, 0.75)),
    "absorbing": volume(AXIS_BOX, (0.5, 0.25, 1.0), (0.0, 0.0, 0.0)),                 # sig_s = 0
    "empty_channel": volume(AXIS_BOX, (0.0, 0.5, 0.25), (0.0, 0.5, 0.75), "hg", 0.3),  # sig_t = 0 on red
}
for _g in G_VALUES:
    VOLUMES[f"hg_{_g!r}"] = volume(TILTED_BOX, (0.125, 0.25, 0.5), (0.5, 0.75, 0.25), "hg", _g)


def add_volume(s, V, **over):
    a = dict(to_world=V["to_world"], sigma_a=V["sig_a"], sigma_s=V["sig_s"], phase=V["phase"], g=V["g"])
    a.update(over)
    return s.add_homogeneous_volume(a.pop("to_world"), a.pop("sigma_a"), a.pop("sigma_s"), **a)


@functools.lru_cache(maxsize=None)
def eval_scene(ctl, name):
    """A floor and the named volume (None: no volume): the scene the evaluators run on."""
    s = ctl.HostScene()
    m = Mesh()
    floor_mesh(m)
    s.add_node(m.add_to(s, [ctl.diffuse_material(*RHO)]))
    s.set_camera((0, 0, 4), (0, 0, 0), (0, 1, 0), 40.0, 64, 64)
    if name is not None:
        assert add_volume(s, VOLUMES[name]) == 0
    return s, s.compile()


def queries(ctl, op, ori, dir_, tmin=0.0, tmax=FLT_MAX, u=(0.0, 0.0), wo=(0.0, 0.0, 0.0)):
    ori = f32(ori).reshape(-1, 3)
    q = np.zeros(ori.shape[0], ctl.MEDIUM_QUERY_DTYPE)
    q["op"] = OPS.index(op)
    q["ori"] = ori
    q["dir"] = f32(dir_)
    q["wo"] = f32(wo)
    q["tmin"] = f32(tmin)
    q["tmax"] = f32(tmax)
    q["u"] = f32(u)
    return q


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return f32(v / np.linalg.norm(v, axis=1)[:, None])


def _unit32(v):
    """fp32 directions of length 1 up to fp32 rounding."""
    v = np.asarray(v, np.float64)
    return f32(v / np.linalg.norm(v, axis=1)[:, None])


def box_centre(V):
    return (V["to_world"].astype(np.float64) @ np.array([0.5, 0.5, 0.5, 1.0]))[:3]


def random_rays(V, n, seed):
    """Origins in a ball of radius 4.5 about the box's centre (the boxes' half diagonals are 3.5), unit
    directions, tmin in [0, 0.5), tmax in [0.5, 8.5) or, for every eighth ray, FLT_MAX."""
    rng = np.random.default_rng(seed)
    r = 4.5 * rng.random(n) ** (1.0 / 3.0)
    ori = f32(box_centre(V) + _unit(rng, n).astype(np.float64) * r[:, None])
    dir_ = _unit(rng, n)
    tmin = f32(0.5 * rng.random(n))
    tmax = f32(0.5 + 8.0 * rng.random(n))
    tmax[::8] = FLT_MAX
    return ori, dir_, tmin, tmax, rng


def random_points(V, n, rng):
    """Points in volume coordinates [-0.25, 1.25]^3: about 30 % inside the box."""
    pl = rng.random((n, 3)) * 1.5 - 0.25
    return f32(pl @ V["to_world"][:3, :3].astype(np.float64).T + V["to_world"][:3, 3])


def op_set(ctl, name, op, n=N_RANDOM, seed=0):
    """(queries, float64 reference) of n random queries of one op on the named volume."""
    V = VOLUMES[name]
    ori, dir_, tmin, tmax, rng = random_rays(V, n, seed + 11 * OPS.index(op))
    if op == "intersect":
        return queries(ctl, op, ori, dir_, tmin, tmax), MR.intersect(V, ori, dir_, tmin, tmax)
    if op == "transmittance":
        return queries(ctl, op, ori, dir_, tmin, tmax), MR.transmittance(V, ori, dir_, tmin, tmax)
    if op == "sample_distance":
        u = f32(rng.random(n))
        u = np.minimum(u, np.nextafter(F(1), F(0)))
        return (queries(ctl, op, ori, dir_, tmin, tmax, u=np.stack([u, np.zeros_like(u)], axis=1)),
                MR.sample_distance(V, ori, dir_, tmin, tmax, u))
    p = random_points(V, n, rng)
    if op == "phase_eval":
        wo = _unit(rng, n)
        return queries(ctl, op, p, dir_, wo=wo), MR.phase_eval(V, p, dir_, wo)
    assert op == "phase_sample"
    u = np.minimum(f32(rng.random((n, 2))), np.nextafter(F(1), F(0)))
    ref = MR.phase_sample(V, dir_, u)
    ref["meets_box"] = MR.intersect(V, p, dir_, np.zeros(n), np.full(n, float(FLT_MAX)))
    return queries(ctl, op, p, dir_, u=u), ref


def random_sets(ctl):
    """(volume name, op, queries, reference): 4096 queries per op on the tilted box, and 512 per op and
    volume on the variants a branch or a coefficient singles out."""
    out = []
    for op in OPS:
        out.append(("tilted_hg", op) + op_set(ctl, "tilted_hg", op))
    for name in ("axis_iso", "absorbing", "empty_channel"):
        for op in OPS:
            out.append((name, op) + op_set(ctl, name, op, 512, seed=100))
    for g in G_VALUES:
        for op in ("phase_eval", "phase_sample"):
            out.append((f"hg_{g!r}", op) + op_set(ctl, f"hg_{g!r}", op, 512, seed=200))
    return out


def edge_rays(ctl, op="intersect"):
    """Rays on AXIS_BOX = [-2, 2]^3 with exact expectations: name -> (queries, hit, t0, t1)."""
    z = (0.0, 0.0, 1.0)
    x = (1.0, 0.0, 0.0)
    cases = {
        # inside: the box is left at +2 along z, 1.5 away
        "starts_inside": ((0.5, -0.25, 0.5), z, 0.0, FLT_MAX, 1, 0.0, 1.5),
        # outside, towards the box: enters at 1, leaves at 5
        "starts_outside": ((0.0, 0.0, -3.0), z, 0.0, FLT_MAX, 1, 1.0, 5.0),
        # outside, away from it
        "points_away": ((0.0, 0.0, 3.0), z, 0.0, FLT_MAX, 0, 0.0, 0.0),
        # on the face z = -2, going in: t0 = 0, t1 = 4
        "on_face_inwards": ((0.0, 0.0, -2.0), z, 0.0, FLT_MAX, 1, 0.0, 4.0),
        # on the face z = 2, going out: the span is empty (t1 = 0 is not > 0)
        "on_face_outwards": ((0.0, 0.0, 2.0), z, 0.0, FLT_MAX, 0, 0.0, 0.0),
        # parallel to the x and y faces, inside their slabs: those axes give -inf / +inf
        "parallel_inside_slab": ((1.0, -1.0, -4.0), z, 0.0, FLT_MAX, 1, 2.0, 6.0),
        # parallel to the x faces, outside their slab
        "parallel_outside_slab": ((3.0, 0.0, -4.0), z, 0.0, FLT_MAX, 0, 0.0, 0.0),
        # the bounds cut the span: [1, 5] against [2, 3]
        "clipped_by_bounds": ((0.0, 0.0, -3.0), z, 2.0, 3.0, 1, 2.0, 3.0),
        # tmax before the box
        "ends_before": ((0.0, 0.0, -3.0), z, 0.0, 0.5, 0, 0.0, 0.0),
        "along_x": ((-4.0, 1.0, 1.0), x, 0.0, FLT_MAX, 1, 2.0, 6.0),
    }
    out = {}
    for name, (o, d, tmin, tmax, hit, t0, t1) in cases.items():
        out[name] = (queries(ctl, op, [o], [d], tmin, tmax), hit, t0, t1)
    return out


def nan_queries(ctl):
    """Every op with a NaN (two payloads, both signs) or an infinity in each input in turn: for the device =
    host comparison only."""
    specials = np.array([0x7fc00000, 0xffc00000, 0x7fc12345, 0xffffffff, 0x7f800000, 0xff800000], np.uint32).view(np.float32)
    rows = []
    for op in OPS:
        base = queries(ctl, op, [(0.25, -0.5, 0.75)], [(0.0, 0.6, 0.8)], 0.0, 4.0, u=(0.25, 0.75), wo=(1.0, 0.0, 0.0))
        for field, width in (("ori", 3), ("dir", 3), ("wo", 3), ("tmin", 0), ("tmax", 0), ("u", 2)):
            for k in range(max(width, 1)):
                for sp in specials:
                    q = base.copy()
                    if width:
                        q[field][0, k] = sp
                    else:
                        q[field][0] = sp
                    rows.append(q)
    # a ray lying in a face's plane and parallel to it: 0 / 0 in the slab test
    rows.append(queries(ctl, "intersect", [(2.0, 0.0, -4.0)], [(0.0, 0.0, 1.0)]))
    rows.append(queries(ctl, "transmittance", [(-2.0, 2.0, -4.0)], [(0.0, 0.0, 1.0)]))
    return np.concatenate(rows)


# ---------------------------------------------------------------------------------------------
# The fog room of the schedule and update tests (and of tools/media_bench.py).
FOG = volume(trs((8.0, 6.0, 8.0), (-4.0, -1.0, -4.0)), (0.05, 0.1, 0.15), (0.3, 0.25, 0.2), "hg", 0.5)


def fog_room(ctl, fog=True, w=64, h=64):
    """A closed room (12 triangles of walls, 2 of a rough conductor card, 2 of an area light), a point light,
    and fog over room and camera."""
    import bsdf_cases as BC
    s = ctl.HostScene()
    rng = np.random.default_rng(5)
    tex = s.add_texture((rng.integers(60, 250, size=(8, 8)).astype(np.uint32) * 0x010101 | 0xff000000).astype(np.uint32),
                        filter=ctl._abi.CTL_TEX_BILINEAR)
    mats = [ctl.diffuse_material(0.6, 0.6, 0.55, texture=tex), ctl.diffuse_material(0.7, 0.7, 0.7),
            ctl.diffuse_material(0.8, 0.8, 0.8), ctl.roughconductor_material(1, BC.GOLD_ETA, BC.GOLD_K, 0.25)]
    m = Mesh()
    (x0, y0, z0), (x1, y1, z1) = (-3.0, 0.0, -3.0), (3.0, 4.0, 3.0)
    # the room's faces look inwards
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
    s.set_camera((0.3, 2.0, -2.75), (0.0, 0.8, 0.0), (0, 1, 0), 60.0, w, h)
    if fog:
        add_volume(s, FOG)
    return s
