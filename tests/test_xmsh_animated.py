"""Animated compiled meshes (.xmsh, MeshCompileType::Animated): the reader, the
writer and the host-side animations against the reference's byte layout
(AnimatedMesh::AnimatedMesh, Engine/AnimatedMesh.cpp:13-66; AnimatedMesh.h:10-67;
md5Compiler.cpp:94-111 writes it).  The reference ships no animated fixture:
the hand-made stream below is assembled field by field from that layout, and the
ribbon grid is compiled by the project's own SBVH builder
(set_animated_bvh(1)), which gives the reference's tree shape: spatial-split
duplicates and leaves of several entries.  tests/test_gpu_anim_xmsh.py runs the
device rebuild on both."""
import ctypes as C
import math
import struct

import numpy as np
import pytest

import oracle
from helpers import oracle_trace, random_rays
from test_anim import _arr, check_tree, grid_frames, oracle_animated, skinned_grid

EMPTY = 0x76543210
XF2 = [1, 0, 0, 25, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]
CAM = ([0, 8, -20], [0, 0, 0], [0, 1, 0], 50)


# ------------------------------------------------------------------ ribbon grid

def ribbon_grid(n=16, ribbons=8, seed=1):
    """skinned_grid(n) plus `ribbons` long thin triangles across the grid's
    square (heights 0.05 + 0.01 i: the SBVH splits them), 9 coincident
    triangles (a leaf cannot separate them), 4 random bone influences on every
    new vertex, and one coordinate overwritten with -0.0 (AABB::Extend's
    min/max chain meets +0.0 there)."""
    V, N, BI, BW, T, UV = skinned_grid(n)
    rng = np.random.default_rng(seed)
    nv, nt = [], []
    base = V.shape[0]
    for i in range(ribbons):
        p, q = rng.uniform(-10, 10, (2, 2))
        h = 0.05 + 0.01 * i
        d = (q - p) / max(1e-6, float(np.linalg.norm(q - p)))
        nv += [[p[0], h, p[1]], [q[0], h, q[1]], [q[0] - 0.05 * d[1], h, q[1] + 0.05 * d[0]]]
        nt.append([base + 3 * i, base + 3 * i + 1, base + 3 * i + 2])
    c0 = base + 3 * ribbons
    nv += [[1.3, 0.3, -2.1], [2.9, 0.35, -2.4], [2.2, 0.4, -0.7]]
    nt += [[c0, c0 + 1, c0 + 2]] * 9
    nv = np.array(nv, np.float32)
    k = nv.shape[0]
    bi = np.zeros((k, 8), np.uint8)
    bi[:, :4] = rng.integers(0, 16, size=(k, 4), dtype=np.uint8)
    bw = np.zeros((k, 8), np.uint8)
    bw[:, :4] = [64, 64, 64, 63]
    V = np.concatenate([V, nv])
    V[n + 3, 1] = -0.0
    N = np.concatenate([N, np.tile(np.array([[0, 1, 0]], np.float32), (k, 1))])
    UV = np.concatenate([UV, ((nv[:, [0, 2]] + 10) / 20).astype(np.float32)])
    return (V, N, np.concatenate([BI, bi]), np.concatenate([BW, bw]), np.concatenate([T, np.array(nt, np.uint32)]),
            UV)


GROUND = np.array([[-14, -1.5, -14], [40, -1.5, -14], [40, -1.5, 14], [-14, -1.5, 14]], np.float32)
LAMP = np.array([[-2, 9, -2], [2, 9, -2], [2, 9, 2], [-2, 9, 2]], np.float32)


def ribbon_frames(t=0.3):
    """Three frames of 16 bones: animate_frame(.., 0, ..) skins between the first
    two, animate_frame(.., 1, ..) between the last two."""
    return np.stack([grid_frames(16, t), grid_frames(16, t + 0.7), grid_frames(16, t + 1.4)])


def _finish(ctl, s, m, w, h):
    """The rest of the ribbon scene around animated mesh m: two instances, a
    ground, a lamp with an area light, the camera."""
    s.add_node(m)
    s.add_node(m, XF2)
    g = s.add_mesh(GROUND, [[0, 2, 1], [0, 3, 2]], [ctl.diffuse_material(0.5, 0.5, 0.5)])
    l = s.add_mesh(LAMP, [[0, 1, 2], [0, 2, 3]], [ctl.diffuse_material(0.0, 0.0, 0.0)])
    s.add_node(g)
    s.add_area_light(s.add_node(l), 0, [20.0, 18.0, 15.0])
    s.set_camera(CAM[0], CAM[1], CAM[2], CAM[3], w, h)


def ribbon_scene(ctl, n=16, ribbons=8, mode=1, w=64, h=48, max_leaf=8):
    """The ribbon grid compiled as the reference compiles a skinned mesh (SBVH on
    the rest pose, leaves up to 8) when mode is 1, with one 3-frame animation."""
    V, N, BI, BW, T, UV = ribbon_grid(n, ribbons)
    s = ctl.HostScene()
    s.set_animated_bvh(mode)
    s.set_bvh_builder("sbvh", 1e-5)
    s.set_bvh_params(0.0, 8, 0, max_leaf)
    m = s.add_animated_mesh(V, N, BI, BW, T, [ctl.diffuse_material(0.7, 0.5, 0.3)], uvs=UV)
    s.add_animation(m, "wave", 24, ribbon_frames())
    _finish(ctl, s, m, w, h)
    return s, s.compile()


def reload_ribbon(ctl, data, w=64, h=48):
    """The same scene with the animated mesh read back from its .xmsh stream."""
    s = ctl.HostScene()
    m = s.add_xmsh(data)
    _finish(ctl, s, m, w, h)
    return s, s.compile()


def mesh_ranges(d, m=0):
    """(node, entry, triangle) ranges of mesh m in the desc's arrays."""
    last = m + 1 == d.n_meshes
    k = d.meshes
    return ((k[m].bvh_node_offset // 4, d.n_bvh_nodes if last else k[m + 1].bvh_node_offset // 4),
            (k[m].bvh_indices_offset, d.n_tri_indices if last else k[m + 1].bvh_indices_offset),
            (k[m].triangle_offset, d.n_tri_data if last else k[m + 1].triangle_offset))


def leaf_sizes(d, m=0):
    """Entries per leaf of mesh m (runs ended by the last-in-leaf flag)."""
    (_, _), (e0, e1), _ = mesh_ranges(d, m)
    idx = _arr(d.tri_indices, C.c_uint32, d.n_tri_indices)[e0:e1]
    ends = np.flatnonzero(idx & 1)
    return np.diff(np.concatenate([[-1], ends]))


def kernel_arrays(d):
    """Every array of the desc a kernel reads for geometry, and the anim_* records."""
    def _arr(ptr, ctype, n):
        if n == 0:
            return np.zeros(0, np.dtype(ctype))
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(n,)).copy()

    out = {
        "tri": _arr(d.tri_data, C.c_uint32, d.n_tri_data * 8),
        "woop": _arr(d.woop_tris, C.c_uint32, d.n_woop_tris * 12),
        "nodes": _arr(d.bvh_nodes, C.c_uint32, d.n_bvh_nodes * 16),
        "idx": _arr(d.tri_indices, C.c_uint32, d.n_tri_indices),
        "mats": bytes(C.string_at(d.materials, d.n_materials * 80)),
        "meshes": bytes(C.string_at(d.meshes, d.n_meshes * 20)),
        "scene_bvh": _arr(d.scene_bvh_nodes, C.c_uint32, d.n_scene_bvh_nodes * 16),
        "mesh_boxes": _arr(d.mesh_boxes, C.c_uint32, d.n_meshes * 6),
        "box": np.array(list(d.box_min) + list(d.box_max), np.float32).view(np.uint32),
        "eps": np.array([d.ray_eps], np.float32).view(np.uint32),
        "light_tris": bytes(C.string_at(d.light_tris, d.n_light_tris * 64)) if d.n_light_tris else b"",
        "anim_vertices": bytes(C.string_at(d.anim_vertices, d.n_anim_vertices * 40)),
        "anim_triangles": _arr(d.anim_triangles, C.c_uint32, d.n_anim_triangles * 3),
        "anim_meshes": bytes(C.string_at(d.anim_meshes, d.n_anim_meshes * 24)),
    }
    return out


def assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], bytes):
            assert a[k] == b[k], k
        else:
            assert np.array_equal(a[k], b[k]), k


# ------------------------------------------------------------ hand-made stream

def _fixed(s, cap):
    return struct.pack("<I", len(s) + 1) + s + b"\0" * (cap - len(s))


def _box(P):
    return P.min(0), P.max(0)


def _node(b0, b1, k0, k1, parent):
    """BVHNodeData: [lo.x hi.x lo.y hi.y] per slot, [lo.z hi.z] per slot, children, parent."""
    (l0, h0), (l1, h1) = b0, b1
    f = struct.pack("<12f", l0[0], h0[0], l0[1], h0[1], l1[0], h1[0], l1[1], h1[1], l0[2], h0[2], l1[2], h1[2])
    return f + struct.pack("<iiii", k0, k1, parent, 0)


HAND_ENTRIES = [0, 1, 2, 3, 4, 5, 6, 7, 3, 8, 9]      # leaf A: 9 entries (triangle 3 twice), leaf B: 2
HAND_ANIMS = [(b"walk", 24, 2), (b"run", 30, 3)]


def hand_frames(frames, joints, seed):
    """Small rigid motions, row-major float4x4."""
    rng = np.random.default_rng(seed)
    out = np.zeros((frames, joints, 4, 4), np.float32)
    for f in range(frames):
        for j in range(joints):
            a = rng.uniform(-0.4, 0.4)
            m = np.eye(4, dtype=np.float32)
            m[0, 0], m[0, 2], m[2, 0], m[2, 2] = math.cos(a), math.sin(a), -math.sin(a), math.cos(a)
            m[:3, 3] = rng.uniform(-0.3, 0.3, 3)
            out[f, j] = m
    return out


def hand_stream(ctl, record=148, joints=2, light=False, bad_index=False):
    """An Animated .xmsh from the reference layout alone: 10 triangles on 30
    vertices with 2 bones; root -> (inner node 1, empty child 0x76543210); node
    1 -> (leaf of 9 entries in which two entries name triangle 3, leaf of 2
    entries); 2 animations of 2 and 3 frames.  Returns the bytes and what they
    were made of.  `cuts` are the tail's section boundaries."""
    L = ctl.lib()
    rng = np.random.default_rng(11)
    nt = 10
    P = (rng.normal(size=(3 * nt, 3)) * 1.5).astype(np.float32)
    P[3 * 8:] += np.float32(4.0)                      # leaf B apart from leaf A
    T = np.arange(3 * nt, dtype=np.uint32).reshape(-1, 3)
    nrm = np.zeros_like(P)
    for t in range(nt):
        a, b, c = P[T[t]]
        g = np.cross(b - a, c - a)
        nrm[T[t]] = (g / np.linalg.norm(g)).astype(np.float32)
    bi = np.zeros((3 * nt, 8), np.uint8)
    bi[:, 1] = 1
    bw = np.zeros((3 * nt, 8), np.uint8)
    bw[:, 0] = rng.integers(0, 256, 3 * nt)
    bw[:, 1] = 255 - bw[:, 0]
    uv = rng.random((3 * nt, 2)).astype(np.float32)
    mi = (np.arange(nt) % 2).astype(np.uint8)
    mats = [ctl.diffuse_material(0.6, 0.5, 0.4), ctl.diffuse_material(0.2, 0.3, 0.8)]
    # TriangleData as the library's own compile writes it for these triangles
    src = ctl.HostScene()
    src.set_bvh_builder("binned").set_bvh_params(0.0, 0)
    src.add_node(src.add_mesh(P, T, mats, mat_index=mi, normals=nrm, uvs=uv))
    src.set_camera(CAM[0], CAM[1], CAM[2], CAM[3], 16, 16)
    sd = src.compile()
    tri = _arr(sd.tri_data, C.c_uint32, nt * 8).reshape(nt, 8)
    woop = b""
    for t in HAND_ENTRIES:
        w = ctl._abi.WoopTri()
        a, b, c = (np.ascontiguousarray(P[i]) for i in T[t])
        L.ctl_woop_set(a.ctypes.data, b.ctypes.data, c.ctypes.data, C.byref(w))
        woop += bytes(w)
    idx = b"".join(struct.pack("<I", (t << 1) | (1 if e in (8, 10) else 0)) for e, t in enumerate(HAND_ENTRIES))
    boxA, boxB = _box(P[:3 * 8]), _box(P[3 * 8:])
    whole = _box(P)
    zero = (np.zeros(3, np.float32), np.zeros(3, np.float32))
    nodes = _node(whole, zero, 4, EMPTY, -1) + _node(boxA, boxB, ~0, ~9, 0)

    out = struct.pack("<I", 1)
    out += struct.pack("<6f", *whole[0], *whole[1])
    if light:
        out += struct.pack("<I", 1) + _fixed(b"glow", 32) + struct.pack("<3f", 6.0, 5.0, 4.0)
    else:
        out += struct.pack("<I", 0)
    out += struct.pack("<I", nt) + tri.tobytes()
    recs = b""
    for nm in (b"base", b"glow"):
        rec = _fixed(nm, 64)
        recs += rec + bytes((0xA5 + i) & 0xff for i in range(record - len(rec)))
    out += struct.pack("<I", 2) + recs
    out += struct.pack("<Q", 2) + nodes
    out += struct.pack("<Q", len(HAND_ENTRIES)) + woop
    out += struct.pack("<Q", len(HAND_ENTRIES)) + idx
    cuts = [len(out)]
    # e_KernelAnimatedMesh {m_uVertexCount, m_uJointCount, m_uAnimCount}
    out += struct.pack("<III", 3 * nt, joints, len(HAND_ANIMS))
    cuts.append(len(out))
    frames = []
    for k, (name, rate, nf) in enumerate(HAND_ANIMS):
        fr = hand_frames(nf, joints, 20 + k)
        frames.append(fr)
        out += struct.pack("<QI", nf, rate) + _fixed(name, 128)       # size_t frames, u32 rate, FixedString<128>
        cuts.append(len(out))
        for f in range(nf):
            out += struct.pack("<Q", joints)                          # AnimationFrame: size_t n
            cuts.append(len(out))
            out += fr[f].tobytes()                                    # n x float4x4
            cuts.append(len(out))
    av = np.zeros(3 * nt, np.dtype([("pos", np.float32, 3), ("normal", np.float32, 3), ("bi", np.uint8, 8),
                                    ("bw", np.uint8, 8)]))
    av["pos"], av["normal"], av["bi"], av["bw"] = P, nrm, bi, bw
    out += av.tobytes()
    cuts.append(len(out))
    tris = T.copy()
    if bad_index:
        tris[-1, 2] = 3 * nt
    out += tris.tobytes()                                             # uint3 per TriangleData
    return out, dict(tri=tri, nodes=nodes, woop=woop, idx=idx, av=av.tobytes(), tris=T, frames=frames, mats=mats,
                     cuts=cuts, box=whole)


def hand_scene(ctl, record=148, w=16, h=16):
    data, parts = hand_stream(ctl, record)
    s = ctl.HostScene()
    m = s.add_xmsh(data, materials=parts["mats"], material_record_size=record)
    s.add_node(m)
    s.add_node(m, [1, 0, 0, 9, 0, 1, 0, 0, 0, 0, 1, 1, 0, 0, 0, 1])
    s.set_camera([2, 2, -14], [2, 1, 0], [0, 1, 0], 50, w, h)
    return s, s.compile(), parts


# ------------------------------------------------------------------------ tests

@pytest.mark.parametrize("record", [148, 1344])
def test_hand_made_animated_stream_loads_as_written(ctl, record):
    """add_xmsh keeps the file's tree, entries and indices byte for byte (the
    9-entry leaf, the repeated triangle and the empty child included), fills the
    anim_* records from the tail and lists the animations."""
    s, d, p = hand_scene(ctl, record)
    assert _arr(d.tri_data, C.c_uint32, d.n_tri_data * 8).tobytes() == p["tri"].tobytes()
    assert _arr(d.bvh_nodes, C.c_uint32, d.n_bvh_nodes * 16).tobytes() == p["nodes"]
    assert _arr(d.woop_tris, C.c_uint32, d.n_woop_tris * 12).tobytes() == p["woop"]
    assert _arr(d.tri_indices, C.c_uint32, d.n_tri_indices).tobytes() == p["idx"]
    assert d.n_woop_tris == 11 and d.n_tri_data == 10
    assert (d.n_anim_meshes, d.n_anim_vertices, d.n_anim_triangles) == (1, 30, 10)
    am = d.anim_meshes[0]
    assert (am.mesh, am.vertex_first, am.vertex_count, am.tri_first, am.tri_count, am.max_bone) == (0, 0, 30, 0, 10, 1)
    assert bytes(C.string_at(d.anim_vertices, 30 * 40)) == p["av"]
    assert np.array_equal(_arr(d.anim_triangles, C.c_uint32, 30).reshape(-1, 3), p["tris"])
    got = s.animations(0)
    assert [(a["name"], a["frame_rate"], a["frames"].shape) for a in got] == \
        [("walk", 24, (2, 2, 4, 4)), ("run", 30, (3, 2, 4, 4))]
    for a, f in zip(got, p["frames"]):
        assert a["frames"].tobytes() == f.tobytes()
    assert list(leaf_sizes(d)) == [9, 2]
    n = _arr(d.bvh_nodes, C.c_int32, 32).reshape(2, 16)
    assert n[0, 13] == EMPTY


def test_write_read_round_trip_animated(ctl):
    """write_animated_xmsh -> add_xmsh -> compile reproduces every kernel array
    and anim_* array of the ribbon-grid scene; the body is write_xmsh's under
    type 1; the reloaded scene writes the same file."""
    s, d = ribbon_scene(ctl)
    assert d.n_woop_tris > d.n_tri_data and leaf_sizes(d).max() >= 3     # reference-shaped
    data = s.write_animated_xmsh(0)
    assert s.write_animated_xmsh(0) == data
    assert struct.unpack_from("<I", data, 0)[0] == 1                    # MeshCompileType::Animated
    static = s.write_xmsh(0)
    assert struct.unpack_from("<I", static, 0)[0] == 0
    assert data[4:len(static)] == static[4:] and len(data) > len(static)
    s2, d2 = reload_ribbon(ctl, data)
    assert_same(kernel_arrays(d), kernel_arrays(d2))
    a, b = s.animations(0), s2.animations(0)
    assert len(a) == len(b) == 1 and a[0]["name"] == b[0]["name"] == "wave" and b[0]["frame_rate"] == 24
    assert a[0]["frames"].tobytes() == b[0]["frames"].tobytes() == ribbon_frames().tobytes()
    assert s2.write_animated_xmsh(0) == data
    with pytest.raises(ctl.CTLError, match="animated"):
        s.write_animated_xmsh(1)                                        # the ground is static


def test_rejects_malformed_animated_streams(ctl):
    good, p = hand_stream(ctl)

    def load(data):
        return ctl.HostScene().add_xmsh(data, materials=p["mats"], material_record_size=148)

    load(good)
    assert len(p["cuts"]) == 2 + 2 + 2 * (2 + 3) + 1
    for cut in p["cuts"]:                                               # every section boundary of the tail
        with pytest.raises(ctl.CTLError, match="animated"):
            load(good[:cut])
    for bad in (good[:-1], good[:p["cuts"][1] + 3]):
        with pytest.raises(ctl.CTLError):
            load(bad)
    with pytest.raises(ctl.CTLError, match="trailing"):
        load(good + b"\0")
    with pytest.raises(ctl.CTLError, match="vertex index"):
        load(hand_stream(ctl, bad_index=True)[0])
    with pytest.raises(ctl.CTLError, match="too few matrices"):
        load(hand_stream(ctl, joints=1)[0])                             # the vertices use bone 1
    with pytest.raises(ctl.CTLError, match="256"):
        load(hand_stream(ctl, joints=257)[0])
    with pytest.raises(ctl.CTLError, match="area light"):
        load(hand_stream(ctl, light=True)[0])
    # the rebuild follows the parent words: a wrong one is refused at the door
    node1 = p["cuts"][0] - (8 + 4 * 11) - (8 + 48 * 11) - 64
    assert struct.unpack_from("<i", good, node1 + 56)[0] == 0
    b = bytearray(good)
    struct.pack_into("<i", b, node1 + 56, 4)
    with pytest.raises(ctl.CTLError, match="parent"):
        load(bytes(b))


def test_animation_frame_index_is_the_float_formula(ctl):
    """ComputeFrameIndex (AnimatedMesh.h:84-91) in float32: inside a frame, exactly
    on a frame, past the last frame."""
    for rate, n, t in [(24, 5, 0.1), (24, 5, 0.125), (24, 5, 1.0), (30, 3, 0.0), (30, 3, 7.77), (24, 2, 100.3),
                       (25, 7, 0.04), (60, 4, 3.999)]:
        a = np.float32(rate) * np.float32(t)
        want = (int(a) % n, np.float32(a - np.floor(a)))
        got = ctl.animation_frame_index(rate, n, t)
        assert got[0] == want[0] and np.float32(got[1]) == want[1], (rate, n, t)
    assert ctl.animation_frame_index(24, 5, 0.125) == (3, 0.0)
    assert ctl.animation_frame_index(24, 5, 1.0)[0] == 4                # frame 24 wraps to 24 % 5
    with pytest.raises(ctl.CTLError):
        ctl.animation_frame_index(24, 0, 0.5)


def test_animated_bvh_mode_0_is_the_binned_build(ctl):
    """set_animated_bvh left at 0: whatever builder the scene selects, the skinned
    mesh compiles with the binned builder and no splits, one entry per triangle
    (the arrays of the same geometry added as a static mesh to a binned scene)."""
    V, N, BI, BW, T, UV = ribbon_grid(16)
    s, d = ribbon_scene(ctl, mode=0)
    ref = ctl.HostScene()
    ref.set_bvh_builder("binned").set_bvh_params(0.0, 0, 0, 8)
    m = ref.add_mesh(V, T, [ctl.diffuse_material(0.7, 0.5, 0.3)], normals=N, uvs=UV)
    _finish(ctl, ref, m, 64, 48)
    dr = ref.compile()
    a, b = kernel_arrays(d), kernel_arrays(dr)
    for k in ("tri", "woop", "nodes", "idx", "scene_bvh", "mesh_boxes", "meshes"):
        assert np.array_equal(a[k], b[k]) if not isinstance(a[k], bytes) else a[k] == b[k], k
    (_, _), (e0, e1), (t0, t1) = mesh_ranges(d)
    assert e1 - e0 == t1 - t0 == T.shape[0]
    assert d.n_woop_tris == d.n_tri_data


@pytest.mark.parametrize("n,ribbons", [(16, 8), (8, 4)])
def test_sbvh_animated_tree_is_valid_and_traverses(ctl, orc, n, ribbons):
    """set_animated_bvh(1): duplicated references and long leaves; the oracle's
    rebuild keeps a valid tree over them (every entry reached once), rotates, and
    traverses to the brute-force hits."""
    s, d = ribbon_scene(ctl, n, ribbons)
    (n0, n1), (e0, e1), (t0, t1) = mesh_ranges(d)
    assert e1 - e0 > t1 - t0                                            # spatial-split duplicates
    assert leaf_sizes(d).max() >= 3
    idx = _arr(d.tri_indices, C.c_uint32, d.n_tri_indices)
    rest = _arr(d.bvh_nodes, C.c_int32, d.n_bvh_nodes * 16).reshape(-1, 16)
    assert check_tree(rest[n0:n1].ravel(), n1 - n0, idx[e0:e1]) == e1 - e0
    F = ribbon_frames()
    keep = None
    for f in (0, 1):
        d2, keep, eps = oracle_animated(ctl, orc, d, F[f], F[f + 1], 0.4, keep)
        tree = keep[2][n0 * 16:n1 * 16].view(np.int32)
        assert check_tree(tree, n1 - n0, idx[e0:e1]) == e1 - e0
        if f == 0:
            assert (tree.reshape(-1, 16)[:, 12:14] != rest[n0:n1, 12:14]).any()   # it rotated
        rays = random_rays(d2, 5000, seed=3 + f)
        t, u, v, tri, node, st = oracle_trace(orc, d2, rays, mode=0)
        bt = np.zeros(rays.shape[0], np.float32)
        btri = np.zeros(rays.shape[0], np.uint32)
        orc.oracle_brute_force(C.byref(d2), rays.shape[0], oracle.ptr(rays), oracle.ptr(bt), oracle.ptr(btri), 0)
        assert (tri != 0xFFFFFFFF).sum() > 500
        assert np.array_equal(t, bt)
        # the 9 coincident triangles are hit at the same distance: which of them is named is the visit order's
        coincident = (btri >= t1 - 9) & (btri < t1)
        assert np.array_equal(tri[~coincident], btri[~coincident])
