"""The deep-stack cases (tests/deep_stack_cases.py) on the host: the oracle's three
visit orders against the exhaustive scan, the stack depth each ray reaches (the
oracle's per-ray output) against ctl_host_bvh_stack_bound -- tight on one level,
one short on two -- and the oracle's own refusal past the product's limit."""
import ctypes as C

import numpy as np
import pytest

import deep_stack_cases as dc
import oracle
from helpers import select_bvh, tie_rule

ORDERS = ("wide", "wideq", "binary")
SINGLE = [("comb", n, 1) for n in dc.DEPTHS] + [("comb", 20, 3), ("comb", 20, 9), ("comb", 128, 3), ("comb", 128, 9)] + \
         [("zigzag", n, 1) for n in dc.ZIGZAG]


def make(ctl, kind, a, b):
    return {"comb": lambda: dc.comb(ctl, a, bottom=b), "zigzag": lambda: dc.zigzag(ctl, a),
            "two_level": lambda: dc.two_level(ctl, a, b)}[kind]()


def trace(orc, case, rays, bvh, any_hit=False):
    """-> (ctl_hit rows, per-ray stack depth) of the oracle in order `bvh`."""
    d = select_bvh(case.desc, bvh)
    n = rays.shape[0]
    hits, depth = np.zeros((n, 4), np.int32), np.zeros(n, np.int32)
    orc.oracle_intersect_depth(C.byref(d), n, oracle.ptr(rays), oracle.ptr(hits), 1 if any_hit else 0, tie_rule(d, orc),
                               0, oracle.ptr(depth))
    return hits, depth


def scan(orc, case, rays):
    """oracle_brute_force (every entry, no tree; it takes eps < t and no tmax) cut to each ray's (tmin, tmax).
    Valid where the closest triangle on a ray's line past eps is the one its (tmin, tmax) leaves: every
    comb family of a one-level case (one triangle per line), and on two levels every family but those
    with a tmin behind a triangle (tmin, mixed)."""
    n = rays.shape[0]
    t, tri = np.zeros(n, np.float32), np.zeros(n, np.uint32)
    orc.oracle_brute_force(C.byref(case.desc), n, oracle.ptr(rays), oracle.ptr(t), oracle.ptr(tri), 0)
    hit = (tri != 0xFFFFFFFF) & (t > rays[:, 3]) & (t < rays[:, 7])
    return hit, t, tri.astype(np.int64)


def check_against_scan(orc, case, name, rays, hits, cut):
    if cut:
        hit, t, tri = scan(orc, case, rays)
    else:
        assert np.all(rays[:, 3] <= np.float32(case.desc.ray_eps)) and np.all(rays[:, 7] > 1e38), name
        hit, t, tri = scan(orc, case, rays)
    assert np.array_equal(hits[:, 2] >= 0, hit), (case.name, name)
    assert np.array_equal(hits[hit, 2], tri[hit]), (case.name, name)
    assert np.array_equal(hits[hit, 0].view(np.float32), t[hit]), (case.name, name)


@pytest.mark.parametrize("kind,a,b", SINGLE, ids=lambda v: str(v))
def test_single_level(ctl, orc, kind, a, b):
    case = make(ctl, kind, a, b)
    bound = ctl.bvh_stack_bound(dc.bvh_array(ctl, case.desc))
    assert bound == case.bounds and max(bound) == case.bound == a      # the depth the case is named for
    for bvh in ORDERS:
        reach = case.reach(bvh)
        for name, (rays, exact) in case.families.items():
            hits, depth = trace(orc, case, rays, bvh)
            check_against_scan(orc, case, name, rays, hits, cut=True)
            assert depth.min() >= 1 and depth.max() <= reach, (bvh, name)     # the bound is safe
            if exact:
                assert np.all(depth == reach), (bvh, name, depth)             # and tight
            if name in ("full", "graded"):
                assert np.all(hits[:, 2] >= 0), (bvh, name)
                want = getattr(case, "zig_hits", np.arange(rays.shape[0])) if name == "full" else np.arange(rays.shape[0])
                assert np.array_equal(hits[:, 2], want), (bvh, name)
            if name == "graded_miss":
                assert np.all(hits[:, 2] < 0)
            if name == "graded" and kind == "comb":
                # one batch walks through every depth up to the bound, the LDS / spill border included
                assert set(range(2, reach + 1)) <= set(depth.tolist()), (bvh, sorted(set(depth.tolist())))
            if name == "mixed":
                assert rays.shape[0] % 64 != 0 and depth.max() == reach and depth.min() <= 2
            if name == "reversed":
                assert depth.max() <= 6       # leaf-first: the far leaf is postponed on a shallow stack
        # the any-hit form of the same queries stays inside the bound too and decides hit / miss alike
        rays = case.families["mixed"][0]
        hits, depth = trace(orc, case, rays, bvh, any_hit=True)
        assert np.array_equal(hits[:, 2] >= 0, scan(orc, case, rays)[0]) and depth.max() <= reach


@pytest.mark.parametrize("k,m", dc.TWO_LEVEL)
def test_two_level(ctl, orc, k, m):
    """top + 1 + mesh is the upload's bound; the deepest stack a ray reaches is one short of it (see
    deep_stack_cases.two_level), in every order."""
    case = dc.two_level(ctl, k, m)
    top = ctl.bvh_stack_bound(dc.scene_bvh_array(ctl, case.desc))
    mesh = ctl.bvh_stack_bound(dc.bvh_array(ctl, case.desc))
    assert top == (k, k) and mesh == (m, m) and case.bound == k + 1 + m
    truth = {name: dc.numpy_scan(case, rays) for name, (rays, _) in case.families.items() if name in ("tmin", "mixed")}
    for bvh in ORDERS:
        reach = case.reach(bvh)
        assert reach == case.bound - 1
        for name, (rays, exact) in case.families.items():
            hits, depth = trace(orc, case, rays, bvh)
            if name in truth:
                # a ray whose nearest triangle lies before its tmin goes on to a later instance: the oracle's
                # scan (closest hit past eps only) cannot answer, an independent float64 scan does
                hit, t, tri, node = truth[name]
                assert np.array_equal(hits[:, 2] >= 0, hit), (bvh, name)
                assert np.array_equal(hits[hit, 2], tri[hit]) and np.array_equal(hits[hit, 1], node[hit]), (bvh, name)
                assert np.allclose(hits[hit, 0].view(np.float32), t[hit], rtol=1e-5, atol=0), (bvh, name)
            else:
                check_against_scan(orc, case, name, rays, hits, cut=name not in ("full", "reversed", "middle", "random"))
            assert depth.min() >= 1 and depth.max() <= reach, (bvh, name)
            if exact:
                assert np.all(depth == reach), (bvh, name, depth)
            if name in ("full", "graded"):
                # ray j hits triangle j of the nearest instance
                assert np.array_equal(hits[:, 2], np.arange(rays.shape[0])) and np.all(hits[:, 1] == 0), (bvh, name)
            if name == "graded_miss":
                assert np.all(hits[:, 2] < 0)
        # the float64 scan against the oracle's own on a family both can answer
        rays = case.families["graded"][0]
        hit, t, tri, node = dc.numpy_scan(case, rays)
        shit, st, stri = scan(orc, case, rays)
        assert np.array_equal(hit, shit) and np.array_equal(tri[hit], stri[hit]) and np.allclose(t[hit], st[hit], rtol=1e-5)


def test_wide_chain_shape(ctl):
    """The 4-wide collapse of a chain: nodes of three leaves and one inner child, which is why the 4-wide
    order stacks three leaves per node and ends at the binary order's depth."""
    case = dc.comb(ctl, 20)
    mesh, wbase, _ = ctl.host_wide_trees(case.desc)
    kids = mesh[:, 24:28].view(np.int32)
    assert wbase[0] == 0 and kids.shape[0] == 7          # ceil(19 inner nodes / 3)
    inner = ((kids >= 0) & (kids != dc.SENT)).sum(axis=1)
    leaves = (kids < 0).sum(axis=1)
    assert np.all(inner[:-1] == 1) and np.all(leaves[:-1] == 3) and inner[-1] == 0
    assert leaves.sum() == 20


@pytest.mark.parametrize("bvh", ORDERS)
def test_oracle_refuses_past_the_limit(ctl, orc, bvh):
    """A tree one entry deeper than the product's stack: the oracle reports a refusal (it used to abort in
    the binary order past 65), and works again afterwards."""
    case = dc.comb(ctl, dc.STACK_MAX + 1)
    assert ctl.bvh_stack_bound(dc.bvh_array(ctl, case.desc)) == (dc.STACK_MAX + 1,) * 2
    rays = case.families["full"][0]
    with pytest.raises(oracle.OracleError, match="deeper traversal stack"):
        trace(orc, case, rays, bvh)
    from helpers import oracle_intersect, oracle_trace      # the entries without the depth output refuse alike
    d = select_bvh(case.desc, bvh)
    with pytest.raises(oracle.OracleError, match="deeper traversal stack"):
        oracle_intersect(orc, d, rays)
    with pytest.raises(oracle.OracleError, match="deeper traversal stack"):
        oracle_trace(orc, d, rays, mode=0, tie=tie_rule(d, orc))
    with pytest.raises(oracle.OracleError, match="deeper traversal stack"):
        orc.oracle_occluded(C.byref(d), rays.shape[0], oracle.ptr(rays), oracle.ptr(np.zeros(rays.shape[0], np.uint8)), 0,
                            tie_rule(d, orc), oracle.CULL_SLAB, 0)
    shallow = case.families["reversed"][0]
    hits, depth = trace(orc, case, shallow, bvh)
    assert np.all(hits[:, 2] >= 0) and depth.max() <= 6
    ok = dc.comb(ctl, dc.STACK_MAX)
    assert np.all(trace(orc, ok, ok.families["full"][0], bvh)[1] == dc.STACK_MAX)


def test_render_cases_go_deep(ctl, orc):
    """The path kernels' own rays on the render cases: the oracle's pass reaches the depth the case is
    named for (oracle_depth_peak), so the GPU passes compared with it do."""
    from helpers import oracle_render
    for case in (dc.comb(ctl, 20, render=True), dc.comb(ctl, 128, render=True), dc.two_level_render(ctl, 39, 87)):
        for bvh in ("wide", "binary"):
            d = select_bvh(case.desc, bvh)
            orc.oracle_depth_peak_reset()
            p = ctl.PTParams(1, 50, 5, 1, 64, 1, 0, 0)
            fb, rays = oracle_render(orc, d, p, 1, d.camera.width, d.camera.height)
            assert orc.oracle_depth_peak() == case.reach(bvh), (case.name, bvh)
            assert rays > d.camera.width * d.camera.height and fb[:, :3].max() > 0.0


def test_light_on_one_of_several_instances_is_refused(ctl):
    """Instances of a mesh share its materials, and an emitting material finds its light through the node
    that was hit: a light on one instance only would leave the others' hits without a light to name
    (found with a 40-instance scene here, whose unlit instances made the path kernels read light
    0xffffffff).  The compiler refuses it."""
    verts, idx = dc.comb_triangles(4)
    s = ctl.HostScene()
    m = s.add_mesh(verts, idx, [ctl.diffuse_material(0.5, 0.5, 0.5)])
    a = s.add_node(m)
    s.add_node(m, tuple(np.eye(4, dtype=np.float32).ravel() + np.float32([0, 0, 0, 9] + [0] * 12)))
    s.add_area_light(a, 0, (1.0, 1.0, 1.0))
    s.set_camera((-5.0, 2.0, 0.0), (0.0, 2.0, 0.0), (0.0, 0.0, 1.0), 40.0, 8, 8)
    with pytest.raises(ctl.CTLError, match="one node only"):
        s.compile()
    s.add_area_light(1, 0, (1.0, 1.0, 1.0))       # a light on each instance: the second node gets no slot either
    with pytest.raises(ctl.CTLError, match="one node only"):
        s.compile()
