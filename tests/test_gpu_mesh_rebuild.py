"""ctl_scene_rebuild_mesh: an uploaded mesh's trees rebuilt on the device from
new positions (csrc/device/lbvh.hip).  Every array the call writes is compared
byte for byte with the numpy restatement (tests/lbvh_ref.py, pinned on the CPU
by test_lbvh_ref.py); traversal and rendering over the rebuilt trees are
compared with the oracle walking the read-back trees."""
import ctypes as C

import numpy as np
import pytest

import oracle
from helpers import binary_bvh, camera_rays, oracle_intersect, oracle_render, random_rays, wide_quant
from lbvh_cases import ALL, add_positions, grid_quads, jittered_grid, mesh, random_tris, restate, single_scene

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENT = 0x76543210


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


_REF = {}


def ref_of(ctl, name):
    if name not in _REF:
        P = mesh(name)
        _REF[name] = (P, restate(ctl, P))
    return _REF[name]


def rebuild(pt, dev, mesh_index, P):
    p = torch.from_numpy(np.ascontiguousarray(P, np.float32)).to(dev)
    pt.rebuild_mesh(mesh_index, p.data_ptr(), P.shape[0])
    return p


def mesh_trees(ctl, pt, n_meshes, m, n, n_wide):
    """The mesh's ranges of the device arrays, located through its read-back record."""
    A = ctl._abi
    rec = pt.read_array(A.CTL_ARRAY_MESHES, 0, n_meshes, np.uint32, 5)[m]
    assert rec[1] % 4 == 0 and rec[2] == 3 * rec[3]
    out = {"rec": rec,
           "nodes": pt.read_array(A.CTL_ARRAY_BVH_NODES, int(rec[1]) // 4, max(n - 1, 1), np.uint32, 16),
           "woop": pt.read_array(A.CTL_ARRAY_WOOP, int(rec[3]), n, np.uint32, 12),
           "idx": pt.read_array(A.CTL_ARRAY_TRI_INDICES, int(rec[3]), n, np.uint32, 1).ravel(),
           "box": pt.read_array(A.CTL_ARRAY_MESH_BOXES, m, 1, np.uint32, 6).ravel()}
    if n_wide is not None:
        wb = int(pt.read_array(A.CTL_ARRAY_MESH_WIDE_BASE, 0, n_meshes, np.uint32, 1)[m, 0])
        out["wide"] = pt.read_array(A.CTL_ARRAY_WIDE_BVH, wb, n_wide, np.uint32, 32)
        out["wbase"] = wb
    return out


def same_bytes(got, R, wide):
    assert np.array_equal(got["idx"], R["idx"])
    assert np.array_equal(got["woop"], R["woop"].view(np.uint32))
    assert np.array_equal(got["nodes"], R["nodes"].view(np.uint32))
    assert np.array_equal(got["box"], R["box"].view(np.uint32))
    if wide:
        assert np.array_equal(got["wide"], R["wide"].view(np.uint32))


@pytest.mark.parametrize("bvh", ["wide", "binary"])
@pytest.mark.parametrize("name", ALL)
def test_rebuild_bytes_equal_the_restatement(ctl, dev, name, bvh):
    """After rebuild_mesh with the uploaded positions: the mesh record, its node, Woop,
    index and 4-wide ranges, its box and the scene's stack bound, byte for byte."""
    P, R = ref_of(ctl, name)
    n = P.shape[0]
    s = single_scene(ctl, P)
    d = s.compile()
    wide = bvh == "wide"
    if not wide:
        d = binary_bvh(d)
    pt = ctl.PathTracer(0)
    try:
        pt.upload_scene(d)
        before = pt.read_array(ctl._abi.CTL_ARRAY_MESHES, 0, 1, np.uint32, 5)[0]
        rebuild(pt, dev, 0, P)
        got = mesh_trees(ctl, pt, 1, 0, n, R["wide"].shape[0] if wide else None)
        assert got["rec"][0] == before[0] and got["rec"][4] == before[4]
        assert got["rec"][1] // 4 >= d.n_bvh_nodes and got["rec"][3] >= d.n_tri_indices   # a region past the upload
        same_bytes(got, R, wide)
        # one instance: no top-level stack
        assert pt.stack_bound() == max(R["bin_bound"], R["wide_bound"] if wide else 0)
    finally:
        pt.close()
        s.close()


# ---- a scene around a rebuilt mesh ---------------------------------------------------------


def wave(P, phase=0.0, amp=0.25):
    """The vertices displaced along z by a sine wave over x and y."""
    V = P.reshape(-1, 3).astype(np.float64).copy()
    V[:, 2] += amp * np.sin(2.3 * V[:, 0] + phase) * np.cos(1.9 * V[:, 1] - phase)
    return np.ascontiguousarray(V.astype(np.float32).reshape(-1, 9))


def build_scene(ctl, w=64, h=48, light_on_mesh=False):
    """Mesh 0 (the one rebuilt: a 2048-triangle heightfield with 40 boxes) under two nodes
    with different transforms, a static ground mesh, an area light on a third mesh."""
    from lbvh_cases import boxes
    P = np.concatenate([grid_quads(32, 32, height=lambda X, Y: 0.2 * np.sin(2 * X) * np.cos(2 * Y)), boxes(40)]).copy()
    s = ctl.HostScene()
    m0 = add_positions(ctl, s, P, ctl.diffuse_material(0.7, 0.5, 0.3))
    G = grid_quads(4, 4, size=14.0)
    G[:, 2::3] = -1.0
    m1 = add_positions(ctl, s, G, ctl.diffuse_material(0.5, 0.5, 0.5))
    L = grid_quads(1, 1, size=2.0)[:, [0, 1, 2, 6, 7, 8, 3, 4, 5]].copy()   # facing down
    L[:, 2::3] = 6.0
    m2 = add_positions(ctl, s, L, ctl.diffuse_material(0.0, 0.0, 0.0))
    n0 = s.add_node(m0)
    s.add_node(m0, [0.8, 0, 0.6, 4.5, 0, 1, 0, 0.5, -0.6, 0, 0.8, 1.0, 0, 0, 0, 1])
    s.add_node(m1)
    nl = s.add_node(m2)
    s.add_area_light(n0 if light_on_mesh else nl, 0, [20.0, 18.0, 15.0])
    s.set_camera([1.5, -9.0, 5.0], [1.5, 0, 0], [0, 0, 1], 50, w, h)
    return s, P


def device_desc(ctl, pt, d, keep):
    """A copy of desc d carrying what the device holds after a rebuild: the whole node, Woop
    and index arrays (regions included), the mesh records, the instance tree, the mesh boxes,
    the scene box and eps; and the device's 4-wide trees for tie_rule(trees=)."""
    A = ctl._abi
    d2 = type(d).from_buffer_copy(d)
    nn, ne = pt.array_size(A.CTL_ARRAY_BVH_NODES), pt.array_size(A.CTL_ARRAY_WOOP)
    assert pt.array_size(A.CTL_ARRAY_TRI_INDICES) == ne
    nodes = pt.read_array(A.CTL_ARRAY_BVH_NODES, 0, nn, np.float32, 16)
    woop = pt.read_array(A.CTL_ARRAY_WOOP, 0, ne, np.float32, 12)
    idx = pt.read_array(A.CTL_ARRAY_TRI_INDICES, 0, ne, np.uint32, 1)
    meshes = pt.read_array(A.CTL_ARRAY_MESHES, 0, d.n_meshes, np.uint32, 5)
    scene = pt.read_array(A.CTL_ARRAY_SCENE_BVH, 0, max(1, d.n_scene_bvh_nodes), np.float32, 16)
    boxes = pt.read_array(A.CTL_ARRAY_MESH_BOXES, 0, d.n_meshes, np.float32, 6)
    sbox = pt.read_array(A.CTL_ARRAY_SCENE_BOX, 0, 1, np.float32, 6).ravel()
    eps = pt.read_array(A.CTL_ARRAY_RAY_EPS, 0, 1, np.float32, 1)[0, 0]
    d2.bvh_nodes = C.cast(nodes.ctypes.data, C.POINTER(A.BVHNode)); d2.n_bvh_nodes = nn
    d2.woop_tris = C.cast(woop.ctypes.data, C.POINTER(A.WoopTri)); d2.n_woop_tris = ne
    d2.tri_indices = C.cast(idx.ctypes.data, C.POINTER(C.c_uint32)); d2.n_tri_indices = ne
    d2.meshes = C.cast(meshes.ctypes.data, C.POINTER(A.KernelMesh))
    d2.scene_bvh_nodes = C.cast(scene.ctypes.data, C.POINTER(A.BVHNode))
    d2.mesh_boxes = C.cast(boxes.ctypes.data, C.POINTER(C.c_float))
    for k in range(3):
        d2.box_min[k] = float(sbox[k])
        d2.box_max[k] = float(sbox[3 + k])
    d2.ray_eps = float(eps)
    trees = None
    if not d.flags & 2:
        nw = pt.array_size(A.CTL_ARRAY_WIDE_BVH)
        trees = (pt.read_array(A.CTL_ARRAY_WIDE_BVH, 0, nw, np.float32, 32),
                 pt.read_array(A.CTL_ARRAY_MESH_WIDE_BASE, 0, d.n_meshes, np.uint32, 1).ravel().copy(),
                 pt.read_array(A.CTL_ARRAY_SCENE_WIDE_BVH, 0, pt.array_size(A.CTL_ARRAY_SCENE_WIDE_BVH), np.float32, 32))
    keep.extend([nodes, woop, idx, meshes, scene, boxes, d, trees])
    return d2, trees, sbox, eps


def gpu_hits(pt, dev, rays):
    r = torch.from_numpy(rays).to(dev)
    hits = torch.zeros((rays.shape[0], 4), dtype=torch.int32, device=dev)
    pt.intersect_buffers(rays.shape[0], r.data_ptr(), hits.data_ptr(), False)
    torch.cuda.synchronize()
    return hits.cpu().numpy()


def ray_set(d2, w, h, n=14000):
    cam = camera_rays(d2, 2 * w, 2 * h // 2, seed=4)
    cam[:, 3] = d2.ray_eps
    return np.ascontiguousarray(np.concatenate([random_rays(d2, n, seed=3, tmin=d2.ray_eps), cam]))


@pytest.mark.parametrize("bvh", ["wide", "binary"])
def test_deformed_mesh_traversal_and_render_equal_the_oracle(ctl, orc, dev, bvh):
    w, h = 64, 48
    s, P = build_scene(ctl, w, h)
    d = s.compile()
    if bvh == "binary":
        d = binary_bvh(d)
    pt = ctl.PathTracer(0)
    keep = []
    try:
        pt.upload_scene(d)
        P2 = wave(P)
        rebuild(pt, dev, 0, P2)
        d2, trees, sbox, eps = device_desc(ctl, pt, d, keep)
        # the mesh's trees are the restatement's for the displaced positions
        R = restate(ctl, P2, wide=bvh == "wide")
        same_bytes(mesh_trees(ctl, pt, d.n_meshes, 0, P2.shape[0], R["wide"].shape[0] if bvh == "wide" else None), R,
                   bvh == "wide")
        # eps = 1e-4 |scene box size|, as scene_eps_kernel computes it (fp32, sum from 0 in x y z order)
        sz = (sbox[3:6] - sbox[0:3]).astype(np.float32)
        q = np.float32(0)
        for k in range(3):
            q = np.float32(q + np.float32(sz[k] * sz[k]))
        assert eps == np.float32(np.float32(1e-4) * np.sqrt(q))
        rays = ray_set(d2, w, h)
        assert rays.shape[0] >= 20000
        want = oracle_intersect(orc, d2, rays, trees=trees)
        got = gpu_hits(pt, dev, rays)
        assert np.array_equal(got, want)
        hit = want[:, 2] != -1
        assert hit.sum() > 5000 and (want[hit, 2] < P.shape[0]).sum() > 2000   # the rebuilt mesh is hit
        bt = np.zeros(rays.shape[0], np.float32)
        btri = np.zeros(rays.shape[0], np.uint32)
        orc.oracle_brute_force(C.byref(d2), rays.shape[0], oracle.ptr(rays), oracle.ptr(bt), oracle.ptr(btri), 0)
        assert (got[:, 0].view(np.float32)[hit] != bt[hit]).sum() <= rays.shape[0] // 1000
        # Occluded over (eps, dist - eps), both forms
        sh = random_rays(d2, 20000, seed=9, tmax=4.0)
        sr = torch.from_numpy(sh).to(dev)
        tie = 0 if bvh == "binary" else oracle.TRAVERSE_WIDE
        for any_hit in (False, True):
            occ = torch.zeros(sh.shape[0], dtype=torch.int32, device=dev)
            pt.occluded(sh.shape[0], sr.data_ptr(), occ.data_ptr(), any_hit)
            torch.cuda.synchronize()
            wo = np.zeros(sh.shape[0], np.uint8)
            orc.oracle_occluded(C.byref(d2), sh.shape[0], oracle.ptr(sh), oracle.ptr(wo), int(any_hit), tie,
                                oracle.CULL_SLAB, 0)
            assert np.array_equal(occ.cpu().numpy().astype(np.uint8), wo)
            assert 200 < wo.sum() < sh.shape[0] - 200
        # two PathTracer passes
        p = ctl.PTParams(1, 50, 5, 1, 64, 1, 0, 0)
        want_fb, wrays = oracle_render(orc, d2, p, 2, w, h, trees=trees)
        fb = torch.zeros((w * h, 7), dtype=torch.float32, device=dev)
        pt.params = p
        pt.reset_rays()
        for k in range(2):
            pt.do_pass(fb.data_ptr(), k)
        torch.cuda.synchronize()
        assert pt.rays_traced() == wrays
        assert np.array_equal(fb.cpu().numpy().view(np.uint32), want_fb.view(np.uint32))
    finally:
        pt.close()
        s.close()


def two_mesh_scene(ctl, PA, PB):
    s = ctl.HostScene()
    a = add_positions(ctl, s, PA)
    b = add_positions(ctl, s, PB)
    s.add_node(a)
    s.add_node(b, [1, 0, 0, 5.0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1])
    s.set_camera([2.5, -1.0, 12.0], [2.5, 0, 0], [0, 1, 0], 40, 32, 32)
    return s


TREE_ARRAYS = ("CTL_ARRAY_BVH_NODES", "CTL_ARRAY_WOOP", "CTL_ARRAY_TRI_INDICES", "CTL_ARRAY_WIDE_BVH")


def test_regions_are_appended_once_and_reused(ctl, dev):
    """array_size grows on the first rebuild of a mesh and never again; the fourth
    rebuild's bytes are a fresh context's first; rebuilding mesh A leaves mesh B alone."""
    A = ctl._abi
    PA, PB = jittered_grid(300, seed=5), random_tris(77, seed=6)
    s = two_mesh_scene(ctl, PA, PB)
    d = s.compile()
    sizes = lambda t: [t.array_size(getattr(A, a)) for a in TREE_ARRAYS]
    pt, pt2 = ctl.PathTracer(0), ctl.PathTracer(0)
    try:
        pt.upload_scene(d)
        up = sizes(pt)
        assert up == [d.n_bvh_nodes, d.n_woop_tris, d.n_tri_indices, ctl.host_wide_trees(d)[0].shape[0]]
        rebuild(pt, dev, 1, PB)
        after_b = sizes(pt)
        assert all(x > y for x, y in zip(after_b, up))
        nwb = restate(ctl, PB)["wide"].shape[0]
        b0 = mesh_trees(ctl, pt, 2, 1, PB.shape[0], nwb)
        poses = [wave(PA, 0.3 * k) for k in range(4)]
        rebuild(pt, dev, 0, poses[0])
        after_a = sizes(pt)
        assert all(x > y for x, y in zip(after_a, after_b))
        recs = []
        for k in range(1, 4):
            rebuild(pt, dev, 0, poses[k])
            assert sizes(pt) == after_a
            recs.append(pt.read_array(A.CTL_ARRAY_MESHES, 0, 2, np.uint32, 5)[0].copy())
        assert not np.array_equal(recs[0], recs[1]) and np.array_equal(recs[0], recs[2])   # the two regions alternate
        R = restate(ctl, poses[3])
        got = mesh_trees(ctl, pt, 2, 0, PA.shape[0], R["wide"].shape[0])
        same_bytes(got, R, True)
        # mesh B: the same record, the same bytes
        b1 = mesh_trees(ctl, pt, 2, 1, PB.shape[0], nwb)
        for k in b0:
            assert np.array_equal(b0[k], b1[k]), k
        # a fresh context's first rebuild of the same positions
        pt2.upload_scene(d)
        rebuild(pt2, dev, 0, poses[3])
        fresh = mesh_trees(ctl, pt2, 2, 0, PA.shape[0], R["wide"].shape[0])
        for k in ("nodes", "woop", "idx", "box", "wide"):
            assert np.array_equal(got[k], fresh[k]), k
    finally:
        pt.close()
        pt2.close()
        s.close()


def test_tree_update_returns_to_the_desc(ctl, orc, dev):
    """update_scene(desc, CTL_DIRTY_BVH) after a rebuild: the hits of the original upload;
    a further rebuild still works."""
    A = ctl._abi
    PA, PB = jittered_grid(300, seed=5), random_tris(77, seed=6)
    s = two_mesh_scene(ctl, PA, PB)
    d = s.compile()
    pt = ctl.PathTracer(0)
    keep = []
    try:
        pt.upload_scene(d)
        rays = random_rays(d, 6000, seed=2, tmin=d.ray_eps)
        first = gpu_hits(pt, dev, rays)
        assert np.array_equal(first, oracle_intersect(orc, d, rays))
        rebuild(pt, dev, 0, wave(PA, 0.7, amp=0.8))
        moved = gpu_hits(pt, dev, rays)
        assert not np.array_equal(moved, first)
        pt.update_scene(d, A.CTL_DIRTY_BVH)
        assert np.array_equal(gpu_hits(pt, dev, rays), first)
        assert pt.array_size(A.CTL_ARRAY_BVH_NODES) == d.n_bvh_nodes
        assert np.array_equal(pt.read_array(A.CTL_ARRAY_MESHES, 0, 2, np.uint32, 5).ravel(),
                              np.ctypeslib.as_array(C.cast(d.meshes, C.POINTER(C.c_uint32)), shape=(10,)))
        P2 = wave(PA, 1.1)
        rebuild(pt, dev, 0, P2)
        d2, trees, _, _ = device_desc(ctl, pt, d, keep)
        assert np.array_equal(gpu_hits(pt, dev, rays), oracle_intersect(orc, d2, rays, trees=trees))
        R = restate(ctl, P2)
        same_bytes(mesh_trees(ctl, pt, 2, 0, PA.shape[0], R["wide"].shape[0]), R, True)
    finally:
        pt.close()
        s.close()


def test_rebuild_drops_a_render_ahead_window(ctl, orc, dev):
    """Inside a CTL_PT_RENDER_AHEAD window the mesh is rebuilt: the next pass renders the
    new geometry (the oracle's pass over the read-back trees), not a pass rendered ahead."""
    w, h = 64, 48
    s, P = build_scene(ctl, w, h)
    d = s.compile()
    pt = ctl.PathTracer(0)
    keep = []
    try:
        pt.upload_scene(d)
        pt.params.flags |= ctl.CTL_PT_RENDER_AHEAD
        fb = torch.zeros((w * h, 7), dtype=torch.float32, device=dev)
        for k in range(4):    # windows of 1, 2 passes, then one of 4 opens at pass 3 (passes 3 .. 6)
            pt.update_scene(d, 0)
            pt.do_pass(fb.data_ptr(), k)
        torch.cuda.synchronize()
        rebuild(pt, dev, 0, wave(P, 0.4, amp=0.6))
        d2, trees, _, _ = device_desc(ctl, pt, d, keep)
        fb.zero_()
        pt.do_pass(fb.data_ptr(), 4)
        torch.cuda.synchronize()
        want = np.zeros((w * h, 7), np.float32)
        oracle_render(orc, d2, pt.params, 1, w, h, fb=want, first_pass=4, trees=trees)
        assert np.array_equal(fb.cpu().numpy().view(np.uint32), want.view(np.uint32))
    finally:
        pt.close()
        s.close()


def test_refusals_leave_the_scene_as_it_was(ctl, orc, dev):
    """Every refusal but the stack bound's (no input of test size reaches it): its message,
    the hits unchanged, the next call succeeding."""
    w, h = 64, 48
    s, P = build_scene(ctl, w, h)
    d = s.compile()
    n = P.shape[0]
    pos = torch.from_numpy(P).to(dev)
    pt = ctl.PathTracer(0)
    keep = []
    try:
        with pytest.raises(ctl.CTLError, match="no scene"):
            pt.rebuild_mesh(0, pos.data_ptr(), n)
        pt.upload_scene(d)
        rebuild(pt, dev, 0, wave(P, 0.2))       # the regions exist: a refusal must not switch them either
        rays = random_rays(d, 6000, seed=2, tmin=d.ray_eps)
        before = gpu_hits(pt, dev, rays)
        rec = pt.read_array(ctl._abi.CTL_ARRAY_MESHES, 0, d.n_meshes, np.uint32, 5).copy()
        bad = P.copy()
        bad[n // 2, 4] = np.nan
        inf = P.copy()
        inf[7, 0] = np.inf
        cases = [("mesh index", lambda: pt.rebuild_mesh(d.n_meshes, pos.data_ptr(), n)),
                 ("triangle count", lambda: pt.rebuild_mesh(0, pos.data_ptr(), n - 1)),
                 ("triangle count", lambda: pt.rebuild_mesh(0, pos.data_ptr(), 0)),
                 ("NULL", lambda: pt.rebuild_mesh(0, None, n)),
                 ("area light", lambda: pt.rebuild_mesh(2, pos.data_ptr(), 2)),
                 ("non-finite", lambda: rebuild(pt, dev, 0, bad)),
                 ("non-finite", lambda: rebuild(pt, dev, 0, inf))]
        for msg, call in cases:
            with pytest.raises(ctl.CTLError, match=msg):
                call()
            pt.sync()       # no render error pending
            assert np.array_equal(pt.read_array(ctl._abi.CTL_ARRAY_MESHES, 0, d.n_meshes, np.uint32, 5), rec), msg
            assert np.array_equal(gpu_hits(pt, dev, rays), before), msg
        P2 = wave(P, 0.9)
        rebuild(pt, dev, 0, P2)
        d2, trees, _, _ = device_desc(ctl, pt, d, keep)
        assert np.array_equal(gpu_hits(pt, dev, rays), oracle_intersect(orc, d2, rays, trees=trees))
        # a quantized scene
        pt.upload_scene(wide_quant(d))
        q_before = gpu_hits(pt, dev, rays)
        with pytest.raises(ctl.CTLError, match="quantized"):
            pt.rebuild_mesh(0, pos.data_ptr(), n)
        pt.sync()
        assert np.array_equal(gpu_hits(pt, dev, rays), q_before)
        pt.upload_scene(d)
        rebuild(pt, dev, 0, P2)
    finally:
        pt.close()
        s.close()


def test_animated_mesh_is_refused(ctl, dev):
    from test_anim import build_scene as anim_scene
    s = anim_scene(ctl)
    d = s.compile()
    pt = ctl.PathTracer(0)
    try:
        pt.upload_scene(d)
        rays = random_rays(d, 4000, seed=2, tmin=d.ray_eps)
        before = gpu_hits(pt, dev, rays)
        nt = d.anim_meshes[0].tri_count
        pos = torch.zeros((nt, 9), dtype=torch.float32, device=dev)
        with pytest.raises(ctl.CTLError, match="animated"):
            pt.rebuild_mesh(d.anim_meshes[0].mesh, pos.data_ptr(), nt)
        pt.sync()
        assert np.array_equal(gpu_hits(pt, dev, rays), before)
        # the static ground mesh of the same scene is rebuilt
        ground = np.array([[-6, -0.5, -6], [6, -0.5, -6], [6, -0.5, 6], [-6, -0.5, 6]], np.float32)
        G = np.concatenate([ground[[0, 2, 1]].ravel(), ground[[0, 3, 2]].ravel()]).reshape(2, 9)
        rebuild(pt, dev, 1, G)
        assert np.array_equal(gpu_hits(pt, dev, rays)[:, 2], before[:, 2])
    finally:
        pt.close()
        s.close()
