"""Scenes and rays that drive the traversal stack (LaneStack, device/traverse.h)
through all of its regimes, up to the 128-entry limit (test infrastructure:
numpy and the host API only, no GPU).

The mesh is a "comb": triangle i lies in the plane x = i + 1 and covers the
strip y in [i, i + 1] (a right triangle (i, -h), (i + 1, -h), (i, h) in (y, z)).
Its compiled BVH is replaced by a hand-made binary chain (the layout of
tests/test_stack_bound.py::chain): node k holds the leaf of the farthest
remaining triangle (child 0) and node k + 1 (child 1), the last node two
leaves; every box spans all of y, so a +x ray walks down child 1 (nearer) and
stacks one leaf per node: a chain over N leaves reaches a stack of exactly N
entries, sentinel included, which is also ctl_host_bvh_stack_bound's figure for
it in the binary and in the 4-wide order.  Ray j = (0, j + 0.5, -h / 2) -> +x
hits triangle j only.

Every builder returns a Case; the Case owns the arrays the edited desc points
to (keep it alive as long as the desc is used)."""
import ctypes as C
import os
import re
import struct

import numpy as np

SENT = 0x76543210
DEPTHS = (13, 14, 15, 16, 17, 18, 19, 20, 33, 64, 65, 66, 127, 128)   # ascending: the first failure is the smallest


def _traverse_h_constants():
    """kLdsStack and kStackMax as the product's header states them (the one place both are read from)."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cudatracerlib_amd", "csrc",
                        "device", "traverse.h")
    text = open(path).read()
    lds = int(re.search(r"#define\s+CTL_LDS_STACK\s+(\d+)", text).group(1))
    top = int(re.search(r"constexpr\s+int\s+kStackMax\s*=\s*(\d+)\s*;", text).group(1))
    return lds, top


LDS_STACK, STACK_MAX = _traverse_h_constants()
FAST_MAX = LDS_STACK - 3     # the 4-wide loops' three-slot fast path runs while sp <= this


def as_f(i):
    return struct.unpack("<f", struct.pack("<i", i))[0]


class Case:
    """An edited desc with the arrays it points to, the stack bound the upload computes for it (bound;
    bounds = its binary and 4-wide parts) and its ray families."""

    def __init__(self, name, desc, keep, bound, n_tris):
        self.name, self.desc, self.keep, self.bound, self.n_tris = name, desc, keep, bound, n_tris
        self.bounds = (bound, bound)
        self.short = 0          # how far the deepest reachable stack stays under the bound (two levels: 1)
        self.families = {}

    def upload_bound(self, bvh):
        """ctl_scene_stack_bound of the desc uploaded for order `bvh`: a CTL_SCENE_BINARY_BVH scene has
        only its binary trees, any other scene the 4-wide trees and the binary ones (stats launches)."""
        return self.bounds[0] if bvh == "binary" else max(self.bounds)

    def reach(self, bvh):
        """The deepest stack a ray can build in order `bvh` ("wide", "wideq", "binary")."""
        return self.bounds[0 if bvh == "binary" else 1] - self.short


# ---------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------
def comb_triangles(n, x0=0.0, half=1.0, mirrored=False):
    """(vertices (3n, 3), indices (n, 3)) of a comb of n triangles from plane x0 + 1 on."""
    v = np.zeros((n, 3, 3), np.float64)
    i = np.arange(n, dtype=np.float64)
    s = -1.0 if mirrored else 1.0       # mirrored: the wide end at z = +half
    v[:, :, 0] = (x0 + i + 1.0)[:, None]
    v[:, 0, 1], v[:, 0, 2] = i, -half * s
    v[:, 1, 1], v[:, 1, 2] = i + 1.0, -half * s
    v[:, 2, 1], v[:, 2, 2] = i, half * s
    return v.reshape(-1, 3).astype(np.float32), np.arange(3 * n, dtype=np.uint32).reshape(n, 3)


def _host_scene(ctl, verts, idx, light_tris=(), camera=None, instances=(None,)):
    """One mesh (diffuse, plus an emitting material on light_tris), one node per instance transform."""
    s = ctl.HostScene()
    mats = [ctl.diffuse_material(0.6, 0.5, 0.4), ctl.diffuse_material(0.8, 0.8, 0.8)]
    mi = np.zeros(idx.shape[0], np.uint8)
    mi[list(light_tris)] = 1
    m = s.add_mesh(verts, idx, mats, mat_index=mi)
    nodes = [s.add_node(m, xf) for xf in instances]
    if len(light_tris):
        s.add_area_light(nodes[0], 1, (20.0, 20.0, 20.0))
    s.set_camera(*camera)
    return s, s.compile()


def _box_of(verts, tris):
    p = verts[np.asarray(tris).ravel()]
    return p.min(axis=0).astype(np.float64), p.max(axis=0).astype(np.float64)


class _Tree:
    """BVHNodeData nodes under construction: children are leaf values (< 0) or node references (index * 4)."""

    def __init__(self):
        self.rows = []

    def node(self, c0, b0, c1, b1):
        (l0, h0), (l1, h1) = b0, b1
        self.rows.append([l0[0], h0[0], l0[1], h0[1], l1[0], h1[0], l1[1], h1[1], l0[2], h0[2], l1[2], h1[2],
                          as_f(c0), as_f(c1), 0.0, 0.0])
        return len(self.rows) - 1

    def chain(self, leaves, boxes):
        """Chain over leaves[0] (nearest) .. leaves[m - 1] (farthest), m >= 2; -> (root reference, box).
        Nodes are emitted root first, so node k + 1 follows node k."""
        m = len(leaves)
        assert m >= 2
        union = [boxes[0]]
        for b in boxes[1:]:
            union.append((np.minimum(union[-1][0], b[0]), np.maximum(union[-1][1], b[1])))
        first = len(self.rows)
        for k in range(m - 1):
            far = m - 1 - k
            if k == m - 2:
                self.node(leaves[1], boxes[1], leaves[0], boxes[0])
            else:
                self.node(leaves[far], boxes[far], (first + k + 1) * 4, union[far - 1])
        return first * 4, union[-1]

    def array(self, ctl):
        arr = (ctl._abi.BVHNode * len(self.rows))()
        for i, r in enumerate(self.rows):
            arr[i].v[:] = r
        return arr


def _entries(ctl, desc, groups):
    """New leaf-entry arrays in the order of `groups` (lists of triangle ids): the Woop record the compiler
    made for each triangle, the last-in-leaf flag on each group's last entry.  -> (woop, idx, first entry
    of each group)."""
    assert desc.n_meshes == 1 and desc.meshes[0].bvh_indices_offset == 0 and desc.meshes[0].bvh_triangle_offset == 0
    old_idx = np.ctypeslib.as_array(desc.tri_indices, (desc.n_tri_indices,))
    old_woop = np.ctypeslib.as_array(C.cast(desc.woop_tris, C.POINTER(C.c_float)), (desc.n_woop_tris, 12))
    where = {}
    for e, w in enumerate(old_idx):
        where.setdefault(int(w) >> 1, e)
    order = [t for g in groups for t in g]
    woop = np.stack([old_woop[where[t]] for t in order]).astype(np.float32)
    idx = np.array([t << 1 for t in order], np.uint32)
    firsts, e = [], 0
    for g in groups:
        firsts.append(e)
        e += len(g)
        idx[e - 1] |= 1
    return np.ascontiguousarray(woop), idx, firsts


def _install(ctl, desc, tree, woop, idx, scene_tree=None):
    """Copy of desc reading the hand-made arrays; -> (desc, the arrays to keep alive)."""
    d = type(desc).from_buffer_copy(desc)
    nodes = tree.array(ctl)
    d.bvh_nodes, d.n_bvh_nodes = C.cast(nodes, C.POINTER(ctl._abi.BVHNode)), len(nodes)
    d.woop_tris, d.n_woop_tris = C.cast(woop.ctypes.data, C.POINTER(ctl._abi.WoopTri)), woop.shape[0]
    d.tri_indices, d.n_tri_indices = C.cast(idx.ctypes.data, C.POINTER(C.c_uint32)), idx.shape[0]
    keep = [nodes, woop, idx]
    if scene_tree is not None:
        sn = scene_tree.array(ctl)
        d.scene_bvh_nodes, d.n_scene_bvh_nodes, d.scene_start_node = C.cast(sn, C.POINTER(ctl._abi.BVHNode)), len(sn), 0
        keep.append(sn)
    return d, keep


def _loose(box, lo_y, hi_y):
    lo, hi = box[0].copy(), box[1].copy()
    lo[1], hi[1] = lo_y, hi_y
    return lo, hi


def _comb_groups(n, bottom):
    """n leaves over n + bottom - 1 triangles: the nearest `bottom` triangles share the bottom leaf."""
    return [list(range(bottom))] + [[bottom - 1 + i] for i in range(1, n)]


def chain_desc(ctl, desc, verts, groups, y_hi, n_leaves=None):
    """desc with its mesh tree replaced by the chain over `groups` (nearest first; only the first n_leaves
    of them if given: the other entries stay in the arrays, outside the tree), boxes loosened to
    y in [0, y_hi]; -> (desc, keep)."""
    woop, idx, firsts = _entries(ctl, desc, groups)
    groups, firsts = groups[:n_leaves], firsts[:n_leaves]
    boxes = [_loose(_box_of(verts, [3 * t + k for t in g for k in range(3)]), 0.0, y_hi) for g in groups]
    tree = _Tree()
    root, _ = tree.chain([~f for f in firsts], boxes)
    assert root == 0
    return _install(ctl, desc, tree, woop, idx)


def _camera(n_y, half, w, h):
    """Far down -x, looking along +x at the comb's middle: near-parallel primary rays that walk the whole chain."""
    dist = 6.0 * max(n_y, 2.0 * half)
    fov = float(np.degrees(2.0 * np.arctan(0.5 * max(n_y, 2.0 * half) / dist)))
    return ((-dist, n_y / 2.0, 0.0), (0.0, n_y / 2.0, 0.0), (0.0, 0.0, 1.0), fov, w, h)


# ---------------------------------------------------------------------------------------------
# rays
# ---------------------------------------------------------------------------------------------
def _rays(o, d, tmin=0.0, tmax=3.0e38):
    o = np.asarray(o, np.float64).reshape(-1, 3)
    r = np.zeros((o.shape[0], 8), np.float32)
    r[:, 0:3] = o
    r[:, 3] = tmin
    r[:, 4:7] = d
    r[:, 7] = tmax
    return r


def _comb_families(case, n_t, half, z=None, x_far=None, xf=None, seed=1):
    """The ray families over a comb of n_t triangles; each entry is (rays, exact).  exact: every ray of
    the family reaches the deepest stack the case allows in the order it is traced in (Case.reach);
    otherwise every ray stays within it.  xf: instance transform applied to the origins (directions stay
    +-x: the instances rotate about x)."""
    z = -half / 2.0 if z is None else z
    x_far = n_t + 2.0 if x_far is None else x_far
    j = np.arange(n_t, dtype=np.float64)
    o = np.stack([np.zeros(n_t), j + 0.5, np.full(n_t, z)], 1)
    o_far = o.copy()
    o_far[:, 0] = x_far
    if xf is not None:
        m = np.asarray(xf, np.float64).reshape(4, 4)
        o = o @ m[:3, :3].T + m[:3, 3]
        o_far = o_far @ m[:3, :3].T + m[:3, 3]
    fam = {}
    fam["full"] = (_rays(o, (1.0, 0.0, 0.0)), True)
    # tmax just behind triangle j: the leaves farther away are culled, ray j stacks about j entries and hits
    fam["graded"] = (_rays(o, (1.0, 0.0, 0.0), tmax=(j + 1.5).astype(np.float32)), False)
    # tmax just in front of triangle j: as shallow, and every ray misses
    fam["graded_miss"] = (_rays(o, (1.0, 0.0, 0.0), tmax=(j + 0.5).astype(np.float32)), False)
    # leaf-first: the far leaf is the nearer child, postponed on a shallow stack
    fam["reversed"] = (_rays(o_far, (-1.0, 0.0, 0.0)), False)
    # tmin behind the nearer half of the comb: those rays lose their triangle
    fam["tmin"] = (_rays(o, (1.0, 0.0, 0.0), tmin=np.float32(n_t // 2 + 0.5)), False)
    fam["tmin_graded"] = (_rays(o, (1.0, 0.0, 0.0), tmin=np.float32(2.5), tmax=(j + 1.5).astype(np.float32)), False)
    mixed = np.concatenate([fam[k][0] for k in ("full", "graded", "graded_miss", "reversed", "tmin", "tmin_graded")])
    rng = np.random.default_rng(seed)
    mixed = mixed[rng.permutation(mixed.shape[0])]
    if mixed.shape[0] % 64 == 0:
        mixed = mixed[:-1]
    fam["mixed"] = (np.ascontiguousarray(mixed), False)
    return fam


def _random_family(desc, n=3000, seed=3):
    from helpers import random_rays
    # tmin = the scene's epsilon: the exhaustive scan the host test compares with takes hits past it only
    return random_rays(desc, n, seed=seed, tmin=float(np.float32(desc.ray_eps))), False


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def comb(ctl, n, bottom=1, render=False, spare=0):
    """Chain of depth n over a comb (bottom: entries of the bottom leaf).  render: triangles as tall as
    the comb is wide, every eighth one an emitter.  spare: further triangles whose entries no leaf of
    the tree names (the geometry arrays of comb(20, spare=109), comb(128, spare=1) and comb(129) are the
    same, only the tree differs)."""
    def make():
        n_in = n + bottom - 1
        n_t = n_in + spare
        half = n_t / 2.0 if render else 1.0
        verts, idx = comb_triangles(n_t, half=half)
        lights = list(range(3, n_t, 8)) if render else ()
        hs, d0 = _host_scene(ctl, verts, idx, lights, _camera(float(n_t), half, 24, 24))
        groups = _comb_groups(n, bottom) + [[t] for t in range(n_in, n_t)]
        d, keep = chain_desc(ctl, d0, verts, groups, float(n_t), n_leaves=n)
        case = Case("comb%d%s%s%s" % (n, "" if bottom == 1 else "_leaf%d" % bottom, "_render" if render else "",
                                      "_spare%d" % spare if spare else ""), d, keep + [hs, d0], n, n_t)
        case.families = _comb_families(case, n_in, half)
        case.families["random"] = _random_family(d)
        return case
    return _cached(("comb", n, bottom, render, spare), make)


def _zigzag(ctl, n, m):
    va, _ = comb_triangles(m)
    vb, _ = comb_triangles(m, x0=m + 1.0, mirrored=True)
    verts = np.concatenate([va, vb])
    idx = np.arange(verts.shape[0], dtype=np.uint32).reshape(-1, 3)
    hs, d0 = _host_scene(ctl, verts, idx, camera=_camera(float(m), 1.0, 24, 24))
    groups = [[t] for t in range(2 * m)]
    woop, eidx, firsts = _entries(ctl, d0, groups)
    boxes = [_loose(_box_of(verts, [3 * t, 3 * t + 1, 3 * t + 2]), 0.0, float(m)) for t in range(2 * m)]
    tree = _Tree()
    tree.rows.append(None)                                    # the root comes first
    ra, ba = tree.chain([~f for f in firsts[:m]], boxes[:m])
    rb, bb = tree.chain([~f for f in firsts[m:]], boxes[m:])
    tree.node(ra, ba, rb, bb)
    tree.rows[0] = tree.rows.pop()
    d, keep = _install(ctl, d0, tree, woop, eidx)
    case = Case("zigzag%d" % n, d, keep + [hs, d0], n, 2 * m)
    case.bounds = (m + 1, n)
    j = np.arange(m, dtype=np.float64)
    o = np.stack([np.zeros(m), j + 0.5, np.full(m, 0.75)], 1)
    case.families["full"] = (_rays(o, (1.0, 0.0, 0.0)), True)
    case.zig_hits = np.arange(m, 2 * m)                       # ray j hits B's triangle j
    lower = _comb_families(case, m, 1.0, x_far=2.0 * m + 3.0)
    for k in ("graded", "reversed", "mixed"):
        case.families[k] = (lower[k][0], False)
    return case


def zigzag(ctl, n):
    """A root over comb A (m leaves, nearer) and comb B (m leaves, behind it, mirrored).  The rays run at
    z = 0.75, above every triangle of A and inside one of B: the stack grows in A (sentinel, B's root,
    A's leaves), every stacked leaf of A is popped and tested down to B's root, then B stacks its leaves
    over the slots A left behind.  Binary order: m + 1 entries in A, then m in B.  The 4-wide collapse
    merges the root with the first nodes of A and B; how depends on m mod 3, and its bound is m + 2 or
    m + 3, never 2 mod 3: m is the one of n - 2, n - 3 for which the scene's bound (the larger of the two
    orders') is n, for the n of ZIGZAG."""
    def make():
        for m in (n - 2, n - 3):
            case = _zigzag(ctl, n, m)
            if max(ctl.bvh_stack_bound(bvh_array(ctl, case.desc))) == n:
                return case
        raise AssertionError("zigzag(%d): no comb length gives that bound" % n)
    return _cached(("zigzag", n), make)


def _rot_x(angle, pivot_y, t):
    """Row-major object->world: rotation about the line (y = pivot_y, z = 0) parallel to x, then translation t."""
    c, s = np.cos(angle), np.sin(angle)
    r = np.array([[1, 0, 0], [0, c, -s], [0, s, c]], np.float64)
    p = np.array([0.0, pivot_y, 0.0])
    m = np.eye(4)
    m[:3, :3] = r
    m[:3, 3] = p - r @ p + np.asarray(t, np.float64)
    return m


def two_level(ctl, k, m):
    """k instances of a comb of depth m, instance i moved (m + 3) * i along x and turned 0.3 * i about its
    own x axis, under a hand-made instance chain (nearest instance at the bottom).  The upload bound is
    top + 1 + mesh = k + 1 + m.  A ray enters an instance from a postponed leaf, and postponing a leaf pops
    the next entry, so the instance level holds at most k - 1 entries at that moment: the deepest stack a
    ray can reach is k + m, one short of the bound (the bound is safe, not tight, on two levels)."""
    def make():
        half = 1.0
        verts, idx = comb_triangles(m, half=half)
        xfs = [_rot_x(0.3 * i, m / 2.0, ((m + 3.0) * i, 0.0, 0.0)) for i in range(k)]
        cam = _camera(float(m), half, 24, 24)
        hs, d0 = _host_scene(ctl, verts, idx, (), cam, [tuple(x.astype(np.float32).ravel()) for x in xfs])
        assert d0.n_nodes == k and d0.n_meshes == 1
        woop, eidx, firsts = _entries(ctl, d0, _comb_groups(m, 1))
        boxes = [_loose(_box_of(verts, [3 * t, 3 * t + 1, 3 * t + 2]), 0.0, float(m)) for t in range(m)]
        tree = _Tree()
        tree.chain([~f for f in firsts], boxes)
        # instance boxes: tight in x, all of the scene box in y and z (every +-x ray meets every instance)
        lo, hi = np.array(d0.box_min[:], np.float64), np.array(d0.box_max[:], np.float64)
        iboxes = []
        for i in range(k):
            bl, bh = lo.copy(), hi.copy()
            bl[0], bh[0] = (m + 3.0) * i + 1.0, (m + 3.0) * i + m
            iboxes.append((bl, bh))
        top = _Tree()
        top.chain([~i for i in range(k)], iboxes)
        d, keep = _install(ctl, d0, tree, woop, eidx, top)
        case = Case("two_level_%dx%d" % (k, m), d, keep + [hs, d0], k + 1 + m, m)
        case.bounds = (k + 1 + m, k + 1 + m)
        case.short = 1
        case.geometry = (verts, [x.astype(np.float32) for x in xfs])     # for numpy_scan
        case.families = _comb_families(case, m, half, x_far=(m + 3.0) * k + 2.0, xf=xfs[0])
        # the same full-depth rays aimed at a middle instance: the instance level holds fewer entries there
        mid = _comb_families(case, m, half, x_far=(m + 3.0) * k + 2.0, xf=xfs[k // 2])
        case.families["middle"] = (mid["full"][0], False)
        case.families["random"] = _random_family(d, n=2000)
        return case
    return _cached(("two_level", k, m), make)


def two_level_render(ctl, k, m):
    """The path kernels' two-level scene: k instances of a comb of depth m (triangles as tall as the comb
    is wide) and, behind them all, an emitting wall: a second mesh under its own node, the farthest leaf
    of the instance chain (an area light belongs to a node's materials, and the instances of one mesh
    share theirs, so the combs carry none).  Bound (k + 1) + 1 + m, reached less one (two_level)."""
    # (an area light on one of several instances of a mesh is not something the host compiler offers)
    def make():
        half = m / 2.0
        verts, idx = comb_triangles(m, half=half)
        # instances 1 .. k - 1 also step aside in y (the instance boxes below still span the scene box, so
        # a ray down the first comb stacks them all): the first comb sees the wall
        xfs = [_rot_x(0.3 * i, m / 2.0, ((m + 3.0) * i, (m + 3.0) * (0 if i == 0 else 1 if i % 2 else -1), 0.0))
               for i in range(k)]
        xw = (m + 3.0) * k + 5.0
        wall = np.array([(xw, -1.0, -half - 1.0), (xw, m + 1.0, -half - 1.0), (xw, m + 1.0, half + 1.0),
                         (xw, -1.0, half + 1.0)], np.float32)
        s = ctl.HostScene()
        mesh = s.add_mesh(verts, idx, [ctl.diffuse_material(0.6, 0.5, 0.4)])
        lmesh = s.add_mesh(wall, np.array([(0, 2, 1), (0, 3, 2)], np.uint32), [ctl.diffuse_material(0.8, 0.8, 0.8)])
        for x in xfs:
            s.add_node(mesh, tuple(x.astype(np.float32).ravel()))
        s.add_area_light(s.add_node(lmesh), 0, (20.0, 20.0, 20.0))
        s.set_camera(*_camera(float(m), half, 24, 24))
        d0 = s.compile()
        assert d0.n_nodes == k + 1 and d0.n_meshes == 2 and d0.meshes[0].bvh_node_offset == 0
        assert d0.meshes[0].bvh_indices_offset == 0 and d0.meshes[0].bvh_triangle_offset == 0
        # the comb's compiled tree and entries come first in the arrays: they are replaced, the wall's
        # follow behind the replacement with their offsets moved
        A = ctl._abi
        n0, e0 = d0.meshes[1].bvh_node_offset // 4, d0.meshes[1].bvh_indices_offset
        assert d0.meshes[1].bvh_triangle_offset == 3 * e0
        old_idx = np.ctypeslib.as_array(d0.tri_indices, (d0.n_tri_indices,))
        old_woop = np.ctypeslib.as_array(C.cast(d0.woop_tris, C.POINTER(C.c_float)), (d0.n_woop_tris, 12))
        old_nodes = np.ctypeslib.as_array(C.cast(d0.bvh_nodes, C.POINTER(C.c_float)), (d0.n_bvh_nodes, 16))
        where = {}
        for e, w in enumerate(old_idx[:e0]):
            where.setdefault(int(w) >> 1, e)
        woop = np.ascontiguousarray(np.concatenate([np.stack([old_woop[where[t]] for t in range(m)]), old_woop[e0:]]),
                                    dtype=np.float32)
        eidx = np.concatenate([np.array([(t << 1) | 1 for t in range(m)], np.uint32), old_idx[e0:]]).astype(np.uint32)
        boxes = [_loose(_box_of(verts, [3 * t, 3 * t + 1, 3 * t + 2]), 0.0, float(m)) for t in range(m)]
        tree = _Tree()
        tree.chain([~t for t in range(m)], boxes)
        n_chain = len(tree.rows)
        tree.rows += [[0.0] * 16 for _ in range(d0.n_bvh_nodes - n0)]      # the wall's nodes, filled in below
        lo, hi = np.array(d0.box_min[:], np.float64), np.array(d0.box_max[:], np.float64)
        iboxes = []
        for i in range(k):
            bl, bh = lo.copy(), hi.copy()
            bl[0], bh[0] = (m + 3.0) * i + 1.0, (m + 3.0) * i + m
            iboxes.append((bl, bh))
        bl, bh = lo.copy(), hi.copy()
        bl[0] = bh[0] = xw
        iboxes.append((bl, bh))
        top = _Tree()
        top.chain([~i for i in range(k + 1)], iboxes)
        d, keep = _install(ctl, d0, tree, woop, eidx, top)
        # the wall's nodes byte for byte (their child words are ints, not floats)
        raw = np.ctypeslib.as_array(C.cast(d.bvh_nodes, C.POINTER(C.c_uint32)), (d.n_bvh_nodes, 16))
        raw[n_chain:] = old_nodes[n0:].view(np.uint32)
        meshes = (A.KernelMesh * 2)()
        for i in range(2):
            C.memmove(C.byref(meshes[i]), C.byref(d0.meshes[i]), C.sizeof(A.KernelMesh))
        meshes[1].bvh_node_offset = 4 * n_chain
        meshes[1].bvh_indices_offset = m
        meshes[1].bvh_triangle_offset = 3 * m
        d.meshes = C.cast(meshes, C.POINTER(A.KernelMesh))
        bound = (k + 1) + 1 + m
        case = Case("two_level_render_%dx%d" % (k, m), d, keep + [s, d0, meshes], bound, m)
        case.bounds = (bound, bound)
        case.short = 1
        return case
    return _cached(("two_level_render", k, m), make)


ZIGZAG = (16, 18, 19, 66, 127)     # bounds the 4-wide collapse of a zigzag can have
TWO_LEVEL = ((5, 11), (6, 11), (20, 43), (21, 43), (40, 87))   # bounds 17, 18, 64, 65, 128


def numpy_scan(case, rays):
    """Closest hit of each ray inside its (tmin, tmax), by Moeller-Trumbore in float64 over every triangle
    of every instance (world-space vertices from the instance transforms): shares no code with the library
    or the oracle.  -> (hit, t, triangle, node)."""
    verts, xfs = case.geometry
    tri = verts.astype(np.float64).reshape(-1, 3, 3)
    world = []
    for x in xfs:
        m = x.astype(np.float64).reshape(4, 4)
        world.append(tri @ m[:3, :3].T + m[:3, 3])
    w = np.stack(world)                                   # (instances, triangles, 3, 3)
    v0, e1, e2 = w[:, :, 0], w[:, :, 1] - w[:, :, 0], w[:, :, 2] - w[:, :, 0]
    n = rays.shape[0]
    best_t, best_tri, best_node = np.full(n, np.inf), np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    for r in range(n):
        o, d = rays[r, 0:3].astype(np.float64), rays[r, 4:7].astype(np.float64)
        p = np.cross(d, e2)
        det = (e1 * p).sum(-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            s0 = o - v0
            u = (s0 * p).sum(-1) * inv
            q = np.cross(s0, e1)
            v = (q * d).sum(-1) * inv
            t = (e2 * q).sum(-1) * inv
        ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > rays[r, 3]) & (t < rays[r, 7])
        if ok.any():
            t = np.where(ok, t, np.inf)
            i = np.unravel_index(np.argmin(t), t.shape)
            best_t[r], best_node[r], best_tri[r] = t[i], i[0], i[1]
    return best_tri >= 0, best_t, best_tri, best_node


def bvh_array(ctl, desc):
    """The desc's mesh nodes as the ctypes array bvh_stack_bound takes."""
    return C.cast(desc.bvh_nodes, C.POINTER(ctl._abi.BVHNode * desc.n_bvh_nodes)).contents


def scene_bvh_array(ctl, desc):
    return C.cast(desc.scene_bvh_nodes, C.POINTER(ctl._abi.BVHNode * desc.n_scene_bvh_nodes)).contents
