"""Meshes of the mesh-rebuild tests (test_lbvh_ref.py, test_gpu_mesh_rebuild.py) as
(n, 9) float32 position arrays (v0 v1 v2 per triangle), scenes around them, and
desc copies that carry restated or read-back trees.  Test infrastructure."""
import ctypes as C

import numpy as np

import lbvh_ref


def grid_quads(nx, ny, jitter=0.0, seed=0, height=None, size=4.0):
    """nx x ny quads (2 triangles each) over [-size/2, size/2]^2 in the xy plane."""
    rng = np.random.default_rng(seed)
    xs = np.linspace(-size / 2, size / 2, nx + 1)
    ys = np.linspace(-size / 2, size / 2, ny + 1)
    X, Y = np.meshgrid(xs, ys, indexing="ij")
    Z = np.zeros_like(X) if height is None else height(X, Y)
    V = np.stack([X, Y, Z], -1)
    if jitter:
        V = V + jitter * (rng.random(V.shape) - 0.5) * (size / max(nx, ny))
    V = V.astype(np.float32)
    a, b, c, d = V[:-1, :-1], V[1:, :-1], V[1:, 1:], V[:-1, 1:]
    t = np.stack([np.concatenate([a, b, c], -1), np.concatenate([a, c, d], -1)], 2)
    return np.ascontiguousarray(t.reshape(-1, 9), np.float32)


def jittered_grid(n, seed=1):
    k = int(np.ceil(np.sqrt(n / 2.0)))
    return grid_quads(k, k, jitter=0.6, seed=seed)[:n].copy()


def random_tris(n, seed=2):
    rng = np.random.default_rng(seed)
    c = rng.random((n, 1, 3)) * 4 - 2
    return (c + rng.random((n, 3, 3)) - 0.5).astype(np.float32).reshape(n, 9)


def boxes(n, seed=3):
    """n small axis-aligned boxes (12 triangles each) above the plane."""
    rng = np.random.default_rng(seed)
    corner = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float64)
    faces = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    out = []
    for _ in range(n):
        o = rng.random(3) * [3.6, 3.6, 0.5] + [-1.8, -1.8, 0.3]
        s = rng.random(3) * 0.3 + 0.05
        v = o + corner * s
        for f in faces:
            out.append(np.concatenate([v[f[0]], v[f[1]], v[f[2]]]))
            out.append(np.concatenate([v[f[0]], v[f[2]], v[f[3]]]))
    return np.array(out, np.float32)


def _hills(X, Y):
    return 0.3 * np.sin(2.1 * X) * np.cos(1.7 * Y) + 0.1 * np.sin(5.0 * X + Y)


def mesh(name):
    if name.startswith("rand"):
        return random_tris(int(name[4:]))
    if name.startswith("grid"):
        return jittered_grid(int(name[4:]))
    if name == "flat":        # the axis-aligned grid: zero extent on z
        return grid_quads(6, 5)
    if name == "coincident":  # nine triangles with one key (and one box), among others
        r = random_tris(20, seed=7)
        return np.concatenate([r[:8], np.repeat(r[8:9], 9, axis=0), r[9:]]).copy()
    if name == "zero_area":
        r = random_tris(31, seed=8)
        r[13, 3:6] = r[13, 0:3] + np.float32(0.25)
        r[13, 6:9] = r[13, 0:3] + np.float32(0.5)     # three collinear points
        return r
    if name == "field3k":     # 2048 + 960 triangles
        return np.concatenate([grid_quads(32, 32, height=_hills), boxes(80)]).copy()
    if name == "field70k":    # 69938 triangles: several blocks of the sort
        return grid_quads(187, 187, height=_hills)
    raise KeyError(name)


SMALL = ["rand1", "rand2", "rand3", "rand5", "grid63", "grid64", "grid65", "grid255", "grid256", "grid257", "grid1025",
         "flat", "coincident", "zero_area", "field3k"]
ALL = SMALL + ["field70k"]


def add_positions(ctl, scene, P, material=None):
    """HostScene.add_mesh of a position array: triangle i = vertices 3 i .. 3 i + 2."""
    P = np.ascontiguousarray(P, np.float32).reshape(-1, 9)
    n = P.shape[0]
    return scene.add_mesh(P.reshape(-1, 3), np.arange(3 * n, dtype=np.uint32).reshape(n, 3),
                          [material or ctl.diffuse_material(0.6, 0.6, 0.6)])


def single_scene(ctl, P, w=32, h=32):
    """The mesh under one node, seen from above."""
    s = ctl.HostScene()
    s.add_node(add_positions(ctl, s, P))
    s.set_camera([0.3, -0.2, 9.0], [0, 0, 0], [0, 1, 0], 40, w, h)
    return s


def desc_with_trees(ctl, d, nodes, woop, idx, meshes=None, keep=None):
    """Copy of desc d whose mesh-tree arrays are the given ones (numpy arrays; kept
    alive in `keep`); meshes = (n_meshes, 5) uint32 records, default: one mesh at 0."""
    A = ctl._abi
    d2 = type(d).from_buffer_copy(d)
    nodes = np.ascontiguousarray(nodes, np.float32)
    woop = np.ascontiguousarray(woop, np.float32)
    idx = np.ascontiguousarray(idx, np.uint32)
    if meshes is None:
        meshes = np.zeros((1, 5), np.uint32)
        meshes[0, 4] = d.meshes[0].std_material_offset
    meshes = np.ascontiguousarray(meshes, np.uint32)
    d2.bvh_nodes = C.cast(nodes.ctypes.data, C.POINTER(A.BVHNode))
    d2.n_bvh_nodes = nodes.size // 16
    d2.woop_tris = C.cast(woop.ctypes.data, C.POINTER(A.WoopTri))
    d2.n_woop_tris = woop.size // 12
    d2.tri_indices = C.cast(idx.ctypes.data, C.POINTER(C.c_uint32))
    d2.n_tri_indices = idx.size
    d2.meshes = C.cast(meshes.ctypes.data, C.POINTER(A.KernelMesh))
    if keep is not None:
        keep.extend([nodes, woop, idx, meshes, d])
    return d2


def restate(ctl, P, wide=True):
    return lbvh_ref.build(P, ctl.woop_set, wide=wide)
