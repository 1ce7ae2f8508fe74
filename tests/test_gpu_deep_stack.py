"""The per-lane traversal stack (LaneStack, device/traverse.h) on the GPU, bit for
bit against the oracle over the scenes of tests/deep_stack_cases.py: stacks on
the 4-wide loops' three-slot fast path, at the top of LDS (14-16 entries), in
the private spill array (17-127) and at the 128-entry limit, on one level and
on two, through ctl_intersect, ctl_intersect_stats, ctl_occluded and the path
kernels.  Every test first asserts, from the oracle's per-ray depth output,
that its rays reach the regime it is about.  A scene one entry past the limit
only ever meets the upload's and the update's refusal."""
import ctypes as C

import numpy as np
import pytest

import deep_stack_cases as dc
import oracle
from adaptive_helpers import masked, prefill, snapshots
from helpers import oracle_render, oracle_trace, select_bvh, tie_rule

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ORDERS = ("wide", "wideq", "binary")
LDS, TOP, FAST = dc.LDS_STACK, dc.STACK_MAX, dc.FAST_MAX
SINGLE = [("comb", n, 1) for n in dc.DEPTHS] + [("comb", 20, 3), ("comb", 20, 9), ("comb", 128, 3), ("comb", 128, 9)] + \
         [("zigzag", n, 1) for n in dc.ZIGZAG]
SCHEDULES = {"persistent": 0, "megakernel": "CTL_PT_MEGAKERNEL", "wavefront": "CTL_PT_WAVEFRONT"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tracer(ctl, dev):
    t = ctl.PathTracer(0)
    yield t
    t.close()


def make(ctl, kind, a, b):
    return {"comb": lambda: dc.comb(ctl, a, bottom=b), "zigzag": lambda: dc.zigzag(ctl, a),
            "two_level": lambda: dc.two_level(ctl, a, b)}[kind]()


def regime(depth):
    """The LaneStack regime a stack of `depth` entries ends in."""
    return "fast" if depth <= FAST else "lds" if depth <= LDS else "spill" if depth < TOP else "limit"


def oracle_hits(orc, desc, rays, any_hit=False):
    n = rays.shape[0]
    hits, depth = np.zeros((n, 4), np.int32), np.zeros(n, np.int32)
    orc.oracle_intersect_depth(C.byref(desc), n, oracle.ptr(rays), oracle.ptr(hits), 1 if any_hit else 0,
                               tie_rule(desc, orc), 0, oracle.ptr(depth))
    return hits, depth


def gpu_hits(tracer, dev, rays, any_hit=False):
    r = torch.from_numpy(rays).to(dev)
    h = torch.zeros((rays.shape[0], 4), dtype=torch.int32, device=dev)
    tracer.intersect_buffers(rays.shape[0], r.data_ptr(), h.data_ptr(), any_hit=any_hit)
    tracer.sync()          # raises if a lane's stack overflowed
    return h.cpu().numpy()


def check_intersect(orc, tracer, dev, case, bvh):
    """Every family, closest and any-hit, against the oracle over the same desc; -> the regimes the
    families' deepest rays ended in."""
    d = select_bvh(case.desc, bvh)
    reach = case.reach(bvh)
    tracer.upload_scene(d)
    assert tracer.stack_bound() == case.upload_bound(bvh)
    seen = set()
    for name, (rays, exact) in case.families.items():
        want, depth = oracle_hits(orc, d, rays)
        assert depth.max() <= reach, (name, depth.max())
        if exact:
            assert np.all(depth == reach), (name, depth)          # the regime the case is named for
        if name == "graded" and case.name.startswith("comb") and reach > LDS:
            assert depth.min() <= FAST and depth.max() > LDS      # one batch on both sides of the LDS border
        if name == "mixed":
            assert rays.shape[0] % 64 and depth.max() == reach and depth.min() <= 2
        seen.add(regime(int(depth.max())))
        got = gpu_hits(tracer, dev, rays)
        bad = np.nonzero((want != got).any(axis=1))[0]
        assert bad.size == 0, (case.name, bvh, name, bad[:8], depth[bad[:8]], want[bad[:4]], got[bad[:4]])
        # any-hit (the rule of test_gpu_parity.test_intersect_any_hit): the oracle's decision, and a real hit
        awant, adepth = oracle_hits(orc, d, rays, any_hit=True)
        assert adepth.max() <= reach
        agot = gpu_hits(tracer, dev, rays, any_hit=True)
        assert np.array_equal(awant[:, 2] >= 0, agot[:, 2] >= 0), (case.name, bvh, name)
        assert np.array_equal(want[:, 2] >= 0, agot[:, 2] >= 0)
        hit = agot[:, 2] >= 0
        t = agot[hit, 0].view(np.float32)
        assert np.all(t >= want[hit, 0].view(np.float32)) and np.all(t < rays[hit, 7]) and np.all(t > rays[hit, 3])
    assert tracer.stack_bound() == case.upload_bound(bvh)
    return seen


@pytest.mark.parametrize("bvh", ORDERS)
@pytest.mark.parametrize("kind,a,b", SINGLE, ids=lambda v: str(v))
def test_intersect_single_level(ctl, orc, tracer, dev, kind, a, b, bvh):
    case = make(ctl, kind, a, b)
    assert case.bound == a
    seen = check_intersect(orc, tracer, dev, case, bvh)
    assert regime(case.reach(bvh)) in seen
    if a == TOP:
        assert "limit" in seen                # a stack of exactly kStackMax entries was traced
    if case.reach(bvh) > LDS:
        assert {"fast", "spill"} <= seen or "limit" in seen


@pytest.mark.parametrize("bvh", ORDERS)
@pytest.mark.parametrize("k,m", dc.TWO_LEVEL)
def test_intersect_two_level(ctl, orc, tracer, dev, k, m, bvh):
    """Bounds 17, 18, 64, 65 and 128 = top + 1 + mesh; the deepest stack a ray reaches on two levels is one
    short of the bound (deep_stack_cases.two_level says why), so 16, 17, 63, 64 and 127: the level switch
    with the pending entry and the mesh sentinel in LDS, across its end and deep in the spill array."""
    case = dc.two_level(ctl, k, m)
    assert case.bound == k + 1 + m and case.reach(bvh) == k + m
    seen = check_intersect(orc, tracer, dev, case, bvh)
    assert regime(k + m) in seen


STAT_CASES = [("comb", 20, 1), ("comb", 66, 1), ("comb", 128, 1), ("comb", 128, 9), ("zigzag", 127, 1), ("two_level", 5, 11),
              ("two_level", 40, 87)]


@pytest.mark.parametrize("kind,a,b", STAT_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("uploaded", ["wide", "binary"])
def test_intersect_stats(ctl, orc, tracer, dev, kind, a, b, uploaded):
    """ctl_intersect_stats runs the binary traverser whatever the scene flag: hits, node, triangle and
    instance counts are the oracle's binary order's."""
    case = make(ctl, kind, a, b)
    d = select_bvh(case.desc, uploaded)
    b_desc = select_bvh(case.desc, "binary")
    tracer.upload_scene(d)
    for name in ("full", "mixed"):
        rays = case.families[name][0]
        want, depth = oracle_hits(orc, b_desc, rays)
        assert depth.max() == case.reach("binary")
        *_, ost = oracle_trace(orc, b_desc, rays, mode=1, tie=0)
        r = torch.from_numpy(rays).to(dev)
        h = torch.zeros((rays.shape[0], 4), dtype=torch.int32, device=dev)
        st = tracer.intersect_stats(rays.shape[0], r.data_ptr(), h.data_ptr())
        tracer.sync()
        assert [int(x) for x in st] == [int(x) for x in ost], (name, st, ost)
        assert np.array_equal(h.cpu().numpy(), want)
    assert tracer.stack_bound() == case.upload_bound(uploaded)


@pytest.mark.parametrize("bvh", ORDERS)
@pytest.mark.parametrize("kind,a,b", [("comb", 16, 1), ("comb", 20, 1), ("comb", 128, 1), ("zigzag", 66, 1),
                                      ("two_level", 6, 11), ("two_level", 40, 87)], ids=lambda v: str(v))
def test_occluded(ctl, orc, tracer, dev, kind, a, b, bvh):
    """ctl_occluded over (eps, tmax - eps), the closest-hit form and the any-hit shadow query."""
    case = make(ctl, kind, a, b)
    d = select_bvh(case.desc, bvh)
    tracer.upload_scene(d)
    full = case.families["full"][0]
    long_rays = full.copy()
    long_rays[:, 7] = np.float32(1.0e4)                    # every triangle in range: the whole chain is walked
    batches = [long_rays] + [case.families[f][0] for f in ("graded", "graded_miss", "mixed") if f in case.families]
    for rays in batches:
        r = torch.from_numpy(rays).to(dev)
        for any_hit in (False, True):
            want, depth = np.zeros(rays.shape[0], np.uint8), np.zeros(rays.shape[0], np.int32)
            orc.oracle_occluded_depth(C.byref(d), rays.shape[0], oracle.ptr(rays), oracle.ptr(want), int(any_hit),
                                      tie_rule(d, orc), oracle.CULL_SLAB, 0, oracle.ptr(depth))
            assert depth.max() <= case.reach(bvh)
            if rays is long_rays:
                assert depth.max() == case.reach(bvh) and want.all()
            occ = torch.zeros(rays.shape[0], dtype=torch.int32, device=dev)
            tracer.occluded(rays.shape[0], r.data_ptr(), occ.data_ptr(), any_hit)
            tracer.sync()
            assert np.array_equal(occ.cpu().numpy().astype(np.uint8), want), (case.name, bvh, any_hit)
    assert 0 < want.sum() < want.size                      # the mixed batch decides both ways
    assert tracer.stack_bound() == case.upload_bound(bvh)


# ---------------------------------------------------------------------------------------------
# the path kernels' own rays
# ---------------------------------------------------------------------------------------------
RENDER = [("comb", 20, 1), ("comb", 66, 1), ("comb", 128, 1), ("two_level", 39, 87)]
_WANT = {}


def render_case(ctl, kind, a, b):
    return dc.comb(ctl, a, render=True) if kind == "comb" else dc.two_level_render(ctl, a, b)


def oracle_pass(ctl, orc, case, bvh, direct, any_hit):
    """Two oracle passes (shared by the schedules) and the deepest stack their rays reached."""
    key = (case.name, bvh, direct, any_hit)
    if key not in _WANT:
        d = select_bvh(case.desc, bvh)
        orc.oracle_depth_peak_reset()
        fb, rays = oracle_render(orc, d, ctl.PTParams(direct, 50, 5, any_hit, 64, 1, 0, 0), 2, d.camera.width,
                                 d.camera.height)
        fb.setflags(write=False)
        _WANT[key] = (fb, rays, orc.oracle_depth_peak())
    return _WANT[key]


@pytest.mark.parametrize("bvh", ORDERS)
@pytest.mark.parametrize("any_hit", [1, 0])
@pytest.mark.parametrize("direct", [1, 0])
@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("kind,a,b", RENDER, ids=lambda v: str(v))
def test_do_pass(ctl, orc, tracer, dev, kind, a, b, schedule, direct, any_hit, bvh):
    case = render_case(ctl, kind, a, b)
    d = select_bvh(case.desc, bvh)
    w, h = d.camera.width, d.camera.height
    want, wrays, peak = oracle_pass(ctl, orc, case, bvh, direct, any_hit)
    assert peak == case.reach(bvh) and regime(peak) in ("spill", "limit")     # the paths' own rays go that deep
    assert want[:, 6].min() == 2 and want[:, :3].max() > 0.0
    flags = SCHEDULES[schedule]
    tracer.upload_scene(d)
    tracer.params = ctl.PTParams(direct, 50, 5, any_hit, 64, 1, 0, getattr(ctl, flags) if flags else 0)
    fb = torch.zeros((w * h, 7), dtype=torch.float32, device=dev)
    tracer.reset_rays()
    for p in range(2):
        tracer.do_pass(fb.data_ptr(), p)
    tracer.sync()
    got = fb.cpu().numpy()
    assert tracer.rays_traced() == wrays
    bad = np.nonzero((want.view(np.uint32) != got.view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, (bad[:10], want[bad[:3]], got[bad[:3]])
    assert tracer.stack_bound() == case.bound


@pytest.mark.parametrize("kind,a,b", RENDER, ids=lambda v: str(v))
def test_block_list_pass(ctl, orc, tracer, dev, kind, a, b):
    """ctl_render_pass_blocks over 16-pixel blocks of the 24 x 24 image (partial blocks on both axes)."""
    case = render_case(ctl, kind, a, b)
    d = case.desc
    w, h, ts, pass_index = d.camera.width, d.camera.height, 16, 2
    p = ctl.PTParams(1, 50, 5, 1, ts, 1, 0, 0)
    pre = prefill(w, h, seed=a)
    orc.oracle_depth_peak_reset()
    snaps, _ = snapshots(orc, d, p, pass_index, pre, 2)
    assert orc.oracle_depth_peak() == case.reach("wide")
    tracer.upload_scene(d)
    tracer.params = p
    for blocks in ([0, 3], [1, 2, 1]):
        fb = torch.from_numpy(pre).to(dev)
        tracer.generate_samples(pass_index)
        tracer.render_pass_blocks(fb.data_ptr(), blocks)
        tracer.sync()
        want = masked(snaps, blocks, w, h, ts)
        assert np.array_equal(fb.cpu().numpy().view(np.uint32), want.view(np.uint32)), blocks


@pytest.mark.parametrize("bvh", ["wide", "binary"])
@pytest.mark.parametrize("kind,a,b", RENDER, ids=lambda v: str(v))
def test_wavefront_path_tracer_pass(ctl, orc, dev, kind, a, b, bvh):
    case = render_case(ctl, kind, a, b)
    d = select_bvh(case.desc, bvh)
    n = d.camera.width * d.camera.height
    want = np.zeros((n, 7), np.float32)
    orc.oracle_depth_peak_reset()
    wrays = orc.oracle_wpt_render_pass(C.byref(d), 1, 12, 3, 1, 1, oracle.ptr(want), tie_rule(d, orc), 0)
    assert orc.oracle_depth_peak() == case.reach(bvh)
    wt = ctl.WavefrontPathTracer(0, direct=True, max_path_length=12, rr_start_depth=3)
    try:
        wt.upload_scene(d)
        fb = torch.zeros((n, 7), dtype=torch.float32, device=dev)
        wt.reset_rays()
        wt.do_pass(fb.data_ptr(), 1, new_trace=True)
        wt.sync()
        assert wt.rays_traced() == wrays and wt.stack_bound() == case.bound
        assert np.array_equal(fb.cpu().numpy().view(np.uint32), want.view(np.uint32))
    finally:
        wt.close()


@pytest.mark.parametrize("kind,a,b", RENDER, ids=lambda v: str(v))
def test_prim_tracer_pass(ctl, orc, dev, kind, a, b):
    case = render_case(ctl, kind, a, b)
    d = case.desc
    n = d.camera.width * d.camera.height
    mode = ctl._abi.PRIM_DRAW_MODES.index("first_f")
    pp = ctl.PrimParams(mode, 7, 1.0, 100000.0, 0)
    want, wdepth = np.zeros((n, 7), np.float32), np.zeros(n, np.float32)
    orc.oracle_depth_peak_reset()
    wrays = orc.oracle_prim_pass(C.byref(d), C.byref(pp), 3, oracle.ptr(want), oracle.ptr(wdepth), tie_rule(d, orc), 0)
    assert orc.oracle_depth_peak() == case.reach("wide")
    pt = ctl.PrimTracer(0, draw_mode=mode)
    try:
        pt.upload_scene(d)
        fb = torch.full((n, 7), 7.0, dtype=torch.float32, device=dev)
        depth = torch.zeros(n, dtype=torch.float32, device=dev)
        pt.reset_rays()
        pt.do_pass(fb.data_ptr(), 3, depth.data_ptr())
        pt.sync()
        assert pt.rays_traced() == wrays and pt.stack_bound() == case.bound
        assert np.array_equal(fb.cpu().numpy().view(np.uint32), want.view(np.uint32))
        assert np.array_equal(depth.cpu().numpy().view(np.uint32), wdepth.view(np.uint32))
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------
# one entry past the limit: refused, never traced
# ---------------------------------------------------------------------------------------------
def trace_all(orc, tracer, dev, case, bvh):
    """The mixed family on the uploaded scene == the oracle over case's desc."""
    d = select_bvh(case.desc, bvh)
    rays = case.families["mixed"][0]
    want, depth = oracle_hits(orc, d, rays)
    assert depth.max() == case.reach(bvh)
    got = gpu_hits(tracer, dev, rays)
    assert np.array_equal(got, want)
    return got


@pytest.mark.parametrize("bvh", ORDERS)
def test_upload_refuses_past_the_limit(ctl, orc, dev, bvh):
    """N = 129 on one level and a two-level bound of 129 are refused by the upload; the context stays
    usable and the scene uploaded before still traces to the same bytes."""
    ok = dc.comb(ctl, 20)
    pt = ctl.PathTracer(0)
    try:
        pt.upload_scene(select_bvh(ok.desc, bvh))
        before = trace_all(orc, pt, dev, ok, bvh)
        for deep in (dc.comb(ctl, TOP + 1), dc.two_level(ctl, 40, 88)):
            assert deep.bound == TOP + 1
            with pytest.raises(ctl.CTLError, match="deeper traversal stack"):
                pt.upload_scene(select_bvh(deep.desc, bvh))
            assert pt.stack_bound() == 20
            assert np.array_equal(trace_all(orc, pt, dev, ok, bvh), before)
        at_limit = dc.comb(ctl, TOP)
        pt.upload_scene(select_bvh(at_limit.desc, bvh))
        assert pt.stack_bound() == TOP
        trace_all(orc, pt, dev, at_limit, bvh)
    finally:
        pt.close()


@pytest.mark.parametrize("bvh", ORDERS)
def test_update_to_the_limit_and_past_it(ctl, orc, dev, bvh):
    """update_scene(CTL_DIRTY_BVH) over one set of geometry arrays (129 triangles): from the chain of
    depth 20 to the chain of depth 128 (reported, traced exactly), and to the chain of depth 129
    (refused; the depth-20 scene stays as it was)."""
    A = ctl._abi
    c20, c128, c129 = dc.comb(ctl, 20, spare=109), dc.comb(ctl, TOP, spare=1), dc.comb(ctl, TOP + 1)
    assert c20.n_tris == c128.n_tris == c129.n_tris == TOP + 1
    for c in (c128, c129):        # only the tree differs
        assert np.array_equal(np.ctypeslib.as_array(c.desc.tri_indices, (TOP + 1,)),
                              np.ctypeslib.as_array(c20.desc.tri_indices, (TOP + 1,)))
    pt = ctl.PathTracer(0)
    try:
        pt.upload_scene(select_bvh(c20.desc, bvh))
        before = trace_all(orc, pt, dev, c20, bvh)
        with pytest.raises(ctl.CTLError, match="deeper traversal stack"):
            pt.update_scene(select_bvh(c129.desc, bvh), A.CTL_DIRTY_BVH)
        assert pt.stack_bound() == 20
        assert np.array_equal(trace_all(orc, pt, dev, c20, bvh), before)
        pt.update_scene(select_bvh(c128.desc, bvh), A.CTL_DIRTY_BVH)
        assert pt.stack_bound() == TOP
        trace_all(orc, pt, dev, c128, bvh)
        with pytest.raises(ctl.CTLError, match="deeper traversal stack"):
            pt.update_scene(select_bvh(c129.desc, bvh), A.CTL_DIRTY_BVH)
        assert pt.stack_bound() == TOP
        trace_all(orc, pt, dev, c128, bvh)
    finally:
        pt.close()
