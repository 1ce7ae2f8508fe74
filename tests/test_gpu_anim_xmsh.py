"""The device rebuild (anim.hip) on reference-shaped animated trees: spatial-split
duplicates, leaves of 3-8 entries, a 9-entry leaf (the 4-wide `count 0 = walk
the flags` code), a triangle named twice in one leaf and an empty child inside
a file's tree; and the resident-animation entry points
(ctl_scene_set_animation / ctl_scene_animate_frame / ctl_scene_animate_time),
k_ComputeState's own signature.  Every array is compared bit for bit with the
oracle's restatement, chained frame to frame as the device's is.  The fixtures
are those of tests/test_xmsh_animated.py."""
import ctypes as C

import numpy as np
import pytest

import oracle
from helpers import binary_bvh, device_wide_trees, oracle_intersect, oracle_render, random_rays
from test_anim import _arr, expected_wide, oracle_animated
from test_xmsh_animated import (EMPTY, hand_scene, leaf_sizes, mesh_ranges, reload_ribbon, ribbon_frames,
                                ribbon_scene)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def six_arrays(ctl, pt, d):
    A = ctl._abi
    return [pt.read_array(A.CTL_ARRAY_TRI_DATA, 0, d.n_tri_data, np.uint32, 8).ravel(),
            pt.read_array(A.CTL_ARRAY_WOOP, 0, d.n_woop_tris, np.uint32, 12).ravel(),
            pt.read_array(A.CTL_ARRAY_BVH_NODES, 0, d.n_bvh_nodes, np.uint32, 16).ravel(),
            pt.read_array(A.CTL_ARRAY_SCENE_BVH, 0, d.n_scene_bvh_nodes, np.uint32, 16).ravel(),
            pt.read_array(A.CTL_ARRAY_MESH_BOXES, 0, d.n_meshes, np.uint32, 6).ravel(),
            pt.read_array(A.CTL_ARRAY_RAY_EPS, 0, 1, np.uint32, 1).ravel()]


NAMES = ["TRI_DATA", "WOOP", "BVH_NODES", "SCENE_BVH", "MESH_BOXES", "RAY_EPS"]


def oracle_six(d, keep, eps):
    tri, woop, nodes, scene, boxes = keep
    return [tri.view(np.uint32), woop.view(np.uint32), nodes.view(np.uint32),
            scene[:d.n_scene_bvh_nodes * 16].view(np.uint32), boxes.view(np.uint32),
            np.array([eps], np.float32).view(np.uint32)]


def assert_six(got, want, tag=""):
    for name, g, w in zip(NAMES, got, want):
        assert np.array_equal(g, w), (name, tag)


@pytest.fixture(scope="module")
def ribbon(ctl):
    """The ribbon grid compiled with the SBVH builder, written as an Animated
    .xmsh and loaded back: (host scene, desc) of the loaded scene."""
    s, d = ribbon_scene(ctl)
    s2, d2 = reload_ribbon(ctl, s.write_animated_xmsh(0))
    (n0, n1), (e0, e1), (t0, t1) = mesh_ranges(d2)
    assert d2.n_woop_tris > d2.n_tri_data and e1 - e0 > t1 - t0      # spatial-split duplicates
    assert leaf_sizes(d2).max() >= 3
    return s2, d2


@pytest.mark.parametrize("bvh", ["wide", "binary"])
def test_loaded_ribbon_grid_animates_bit_exact(ctl, orc, dev, ribbon, bvh):
    """upload_animations, then animate_frame for two successive poses (the second
    from the first's tree) on a tree with duplicated references and leaves of 1
    to 8 entries: the six arrays equal the oracle's, the 4-wide copy equals its
    upload topology refit from the oracle's leaf boxes."""
    s, d = ribbon
    if bvh == "binary":
        d = binary_bvh(d)
    F = ribbon_frames()
    pt = ctl.PathTracer(0)
    try:
        pt.upload_scene(d)
        upload = None if bvh == "binary" else pt.wide_trees(d)
        pt.upload_animations(s)
        pt.animate_frame(0, 0, 0, 0.4)
        pt.animate_frame(0, 0, 1, 0.4)
        d2, keep, eps = oracle_animated(ctl, orc, d, F[0], F[1], 0.4)
        (n0, n1), _, _ = mesh_ranges(d)
        rest = _arr(d.bvh_nodes, C.c_int32, d.n_bvh_nodes * 16).reshape(-1, 16)
        first = keep[2].view(np.int32).reshape(-1, 16)
        assert (first[n0:n1, 12:14] != rest[n0:n1, 12:14]).any()     # the oracle's first frame rotated
        d2, keep, eps = oracle_animated(ctl, orc, d, F[1], F[2], 0.4, keep)
        assert_six(six_arrays(ctl, pt, d), oracle_six(d, keep, eps))
        if upload is not None:
            mesh, wbase, _ = pt.wide_trees(d)
            want = expected_wide(upload[0], upload[1], d, keep[2])
            assert np.array_equal(mesh.view(np.uint32), want.view(np.uint32))
    finally:
        pt.close()


@pytest.mark.parametrize("bvh", ["wide", "binary"])
def test_loaded_ribbon_grid_traversal_and_render_bit_exact(ctl, orc, dev, ribbon, bvh):
    """The rebuilt trees traverse to the oracle's hits on the oracle's animated
    arrays, the hit distances equal brute force, a 2-pass render is bit-exact."""
    w, h = 64, 48
    s, d = ribbon
    if bvh == "binary":
        d = binary_bvh(d)
    F = ribbon_frames()
    pt = ctl.PathTracer(0)
    try:
        pt.upload_scene(d)
        pt.upload_animations(s)
        pt.animate_frame(0, 0, 0, 0.6)
        d2, keep, eps = oracle_animated(ctl, orc, d, F[0], F[1], 0.6)
        rays = random_rays(d2, 20000, seed=3, tmin=d2.ray_eps)
        trees = None if bvh == "binary" else device_wide_trees(pt, d)
        want = oracle_intersect(orc, d2, rays, trees=trees)
        r = torch.from_numpy(rays).to(dev)
        hits = torch.zeros((rays.shape[0], 4), dtype=torch.int32, device=dev)
        pt.intersect_buffers(rays.shape[0], r.data_ptr(), hits.data_ptr(), False)
        torch.cuda.synchronize()
        got = hits.cpu().numpy()
        assert np.array_equal(got, want)
        hit = want[:, 2] != -1
        assert hit.sum() > 1000
        bt = np.zeros(rays.shape[0], np.float32)
        btri = np.zeros(rays.shape[0], np.uint32)
        orc.oracle_brute_force(C.byref(d2), rays.shape[0], oracle.ptr(rays), oracle.ptr(bt), oracle.ptr(btri), 0)
        assert np.array_equal(got[:, 0].view(np.float32)[hit], bt[hit])
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


@pytest.mark.parametrize("bvh", ["wide", "binary"])
def test_hand_made_stream_animates_bit_exact(ctl, orc, dev, bvh):
    """The 9-entry leaf (a 4-wide `count 0` leaf), the triangle named twice in it
    and the root's empty child, through two animate_frame calls: the first wraps
    from the last frame of the 3-frame animation to its first."""
    s, d, p = hand_scene(ctl, 1344)
    assert list(leaf_sizes(d)) == [9, 2]
    assert _arr(d.bvh_nodes, C.c_int32, 32)[13] == EMPTY
    if bvh == "binary":
        d = binary_bvh(d)
    run, walk = p["frames"][1], p["frames"][0]
    pt = ctl.PathTracer(0)
    try:
        pt.upload_scene(d)
        upload = None if bvh == "binary" else pt.wide_trees(d)
        if upload is not None:
            codes = ~upload[0].view(np.int32)[:, 24:28]
            leaf = upload[0].view(np.int32)[:, 24:28] < 0
            assert ((codes & 7) == 0)[leaf].any()                    # the 9-entry leaf is a walk-the-flags leaf
        pt.upload_animations(s)
        pt.animate_frame(0, 1, 2, 0.3)
        pt.animate_frame(0, 0, 0, 0.7)
        d2, keep, eps = oracle_animated(ctl, orc, d, run[2], run[0], 0.3)
        d2, keep, eps = oracle_animated(ctl, orc, d, walk[0], walk[1], 0.7, keep)
        assert_six(six_arrays(ctl, pt, d), oracle_six(d, keep, eps))
        assert not np.array_equal(keep[1].view(np.uint32), _arr(d.woop_tris, C.c_uint32, d.n_woop_tris * 12))
        if upload is not None:
            mesh, wbase, _ = pt.wide_trees(d)
            want = expected_wide(upload[0], upload[1], d, keep[2])
            assert np.array_equal(mesh.view(np.uint32), want.view(np.uint32))
        rays = random_rays(d2, 4000, seed=9, tmin=d2.ray_eps)
        trees = None if bvh == "binary" else device_wide_trees(pt, d)
        want = oracle_intersect(orc, d2, rays, trees=trees)
        r = torch.from_numpy(rays).to(dev)
        hits = torch.zeros((rays.shape[0], 4), dtype=torch.int32, device=dev)
        pt.intersect_buffers(rays.shape[0], r.data_ptr(), hits.data_ptr(), False)
        torch.cuda.synchronize()
        assert np.array_equal(hits.cpu().numpy(), want)
        assert (want[:, 2] != -1).sum() > 100
    finally:
        pt.close()


@pytest.mark.parametrize("bvh", ["wide", "binary"])
def test_short_leaves_with_duplicates_animate_bit_exact(ctl, orc, dev, bvh):
    """max_leaf 3: duplicated references and a few 3-entry leaves at a mean of 2
    entries per leaf, where the Woop phase runs one thread per leaf (the trees
    above run it per entry); host frames through animate, two chained poses."""
    s, d = ribbon_scene(ctl, 8, 4, max_leaf=3)
    (n0, n1), (e0, e1), (t0, t1) = mesh_ranges(d)
    sizes = leaf_sizes(d)
    assert e1 - e0 > t1 - t0 and sizes.max() == 3 and e1 - e0 < 3 * sizes.size
    if bvh == "binary":
        d = binary_bvh(d)
    F = ribbon_frames()
    pt = ctl.PathTracer(0)
    try:
        pt.upload_scene(d)
        upload = None if bvh == "binary" else pt.wide_trees(d)
        pt.animate(0, F[0], F[1], 0.4)
        pt.animate(0, F[1], F[2], 0.4)
        d2, keep, eps = oracle_animated(ctl, orc, d, F[0], F[1], 0.4)
        d2, keep, eps = oracle_animated(ctl, orc, d, F[1], F[2], 0.4, keep)
        assert_six(six_arrays(ctl, pt, d), oracle_six(d, keep, eps))
        if upload is not None:
            mesh, wbase, _ = pt.wide_trees(d)
            want = expected_wide(upload[0], upload[1], d, keep[2])
            assert np.array_equal(mesh.view(np.uint32), want.view(np.uint32))
    finally:
        pt.close()


@pytest.mark.parametrize("bvh", ["wide", "binary"])
def test_entry_points_leave_the_same_bytes(ctl, dev, bvh):
    """animate_frame(m, a, f, lerp) == animate(m, frames[f], frames[(f + 1) % n], lerp)
    in a second context (f the last frame: the wrap), and animate_time == animate_frame
    at the indices ctl_animation_frame_index returns, for a t inside the animation
    and one past its last frame."""
    s, d = ribbon_scene(ctl, 8, 4)
    if bvh == "binary":
        d = binary_bvh(d)
    F = ribbon_frames()
    x, y = ctl.PathTracer(0), ctl.PathTracer(0)
    try:
        for pt in (x, y):
            pt.upload_scene(d)
            pt.upload_animations(s)

        def same(tag):
            assert_six(six_arrays(ctl, x, d), six_arrays(ctl, y, d), tag)
            if bvh == "wide":
                assert np.array_equal(x.wide_trees(d)[0].view(np.uint32), y.wide_trees(d)[0].view(np.uint32)), tag

        rest = six_arrays(ctl, x, d)
        x.animate_frame(0, 0, 2, 0.25)
        y.animate(0, F[2], F[0], 0.25)
        same("frame 2 -> 0")
        assert not np.array_equal(six_arrays(ctl, x, d)[1], rest[1])  # it moved
        for t in (0.06, 0.2):                                         # 24 fps, 3 frames: a = 1.44, 4.8
            frame, lerp = ctl.animation_frame_index(24, 3, t)
            x.animate_time(0, 0, t)
            y.animate_frame(0, 0, frame, lerp)
            same(t)
        assert ctl.animation_frame_index(24, 3, 0.2)[0] == 4 % 3      # past the last frame
    finally:
        x.close()
        y.close()


def test_resident_animation_refusals(ctl, dev):
    s, d = ribbon_scene(ctl, 8, 4)
    pt = ctl.PathTracer(0)
    try:
        pt.upload_scene(d)
        with pytest.raises(ctl.CTLError, match=r"status 1\).*resident"):
            pt.animate_frame(0, 0, 0, 0.5)                            # before set_animation
        with pytest.raises(ctl.CTLError, match=r"status 1\).*resident"):
            pt.animate_time(0, 0, 0.5, frame_rate=24)
        pt.upload_animations(s)
        with pytest.raises(ctl.CTLError, match=r"status 1\).*n_frames"):
            pt.animate_frame(0, 0, 3, 0.5)                            # 3 frames
        with pytest.raises(ctl.CTLError, match=r"status 1\).*mesh index"):
            pt.animate_frame(1, 0, 0, 0.5)                            # one animated mesh
        few = ribbon_frames()[:, :8]                                  # the vertices use bones up to 15
        with pytest.raises(ctl.CTLError, match=r"status 1\).*bone"):
            pt.set_animation(0, 1, few)
        with pytest.raises(ctl.CTLError, match=r"status 1\).*256"):
            pt.set_animation(0, 1, np.zeros((1, 257, 4, 4), np.float32))
        pt.animate_frame(0, 0, 2, 0.5)                                # still usable
        pt.upload_scene(d)                                            # the tables go with the scene
        with pytest.raises(ctl.CTLError, match=r"status 1\).*resident"):
            pt.animate_frame(0, 0, 0, 0.5)
    finally:
        pt.close()
