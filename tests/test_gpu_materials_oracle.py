"""The kShadeMat kernels against the oracle's restatement of the five material types, bit for bit:
the three PathTracer schedules, render_passes and rank shards, the block-list pass, the
WavefrontPathTracer and the PrimTracer, on scene A (one mesh, one node: the single-instance
kernels) and scene B (two meshes under two nodes: the multi-instance kernels, ext records behind a
material_offset, the inside of glass, emitters seen through specular bounces).  Framebuffers are
compared as uint32 and the ray counts must be equal; there is no tolerance anywhere in this file.
tests/test_oracle_materials.py shows on the CPU that the two scenes reach the branches meant."""
import ctypes as C

import numpy as np
import pytest
import torch

import materials_scenes as MS
import oracle
from adaptive_helpers import masked, prefill, snapshots
from helpers import select_bvh, tie_rule

pytestmark = pytest.mark.gpu
W, H = MS.W, MS.H


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


def exact(got, want, w=W):
    assert MS.same(got, want), MS.first_differences(got, want, w)


def schedule_flags(ctl, schedule):
    return {"persistent": 0, "megakernel": ctl.CTL_PT_MEGAKERNEL, "wavefront": ctl.CTL_PT_WAVEFRONT}[schedule]


def render_gpu(tracer, dev, desc, params, passes, w=W, h=H, first_pass=0):
    tracer.upload_scene(desc)
    tracer.params = params
    fb = torch.zeros((w * h, 7), dtype=torch.float32, device=dev)
    tracer.reset_rays()
    for p in range(first_pass, first_pass + passes):
        tracer.do_pass(fb.data_ptr(), p)
    torch.cuda.synchronize()
    return fb.cpu().numpy(), tracer.rays_traced()


PT_CASES = ([(s, d, sch, bvh, "std") for s in "AB" for d in (1, 0) for sch in ("persistent", "wavefront", "megakernel")
             for bvh in ("wide", "binary")]
            + [(s, 1, "persistent", "wideq", "std") for s in "AB"]
            + [("B", d, sch, "wide", "long") for d in (1, 0) for sch in ("persistent", "wavefront", "megakernel")])


@pytest.mark.parametrize("name,direct,schedule,bvh,render", PT_CASES)
def test_path_tracer_equals_the_oracle(ctl, tracer, dev, name, direct, schedule, bvh, render):
    """PathTrace<DIRECT> through shade_hit over every schedule and node layout: v.specular, the RR
    rule after a delta bounce, the MIS weight after one, NEE's type mask and the ext record's index
    are all in the image; "long" cuts paths inside the glass at 50 with roulette from the second hit."""
    want, wrays, _ = MS.reference(name, direct, bvh, render)
    d = select_bvh(MS.scene(name)[1], bvh)
    got, grays = render_gpu(tracer, dev, d, MS.pt_params(ctl, direct, render, schedule_flags(ctl, schedule)),
                            MS.RENDERS[render][2])
    assert grays == wrays
    exact(got, want)


@pytest.mark.parametrize("direct", [1, 0])
def test_render_passes_and_rank_shards_of_scene_b(ctl, orc, tracer, dev, direct):
    """render_passes(first = 5, n = 3) is the oracle's passes 5, 6, 7; three rank shards sum to the
    1-rank image and rank 1's part is the oracle's rank render."""
    d = MS.scene("B")[1]
    first, n, ranks = 5, 3, 3
    p = MS.pt_params(ctl, direct)
    want = np.zeros((W * H, 7), np.float32)
    wrays = 0
    for k in range(first, first + n):
        wrays += orc.oracle_render_pass(C.byref(d), C.byref(p), k, oracle.ptr(want), tie_rule(d, orc), 0, 1, None)
    tracer.upload_scene(d)
    tracer.params = p
    fb = torch.zeros((W * H, 7), dtype=torch.float32, device=dev)
    tracer.reset_rays()
    tracer.render_passes(fb.data_ptr(), first, n)
    torch.cuda.synchronize()
    assert tracer.rays_traced() == wrays
    full = fb.cpu().numpy()
    exact(full, want)
    acc = np.zeros_like(full)
    for r in range(ranks):
        pr = MS.pt_params(ctl, direct, num_ranks=ranks, rank=r)
        part, _ = render_gpu(tracer, dev, d, pr, n, first_pass=first)
        acc += part
        if r == 1:
            rank_want = np.zeros_like(full)
            for k in range(first, first + n):
                orc.oracle_render_pass(C.byref(d), C.byref(pr), k, oracle.ptr(rank_want), tie_rule(d, orc), 0, 1, None)
            assert 0 < (rank_want[:, 6] > 0).sum() < (full[:, 6] > 0).sum()
            exact(part, rank_want)
    exact(acc, full)


def test_block_list_pass_on_scene_a(ctl, orc, tracer, dev):
    """ctl_render_pass_blocks with the kShadeMat kernel: scene A at 96 x 64 in 32-pixel blocks, Direct 1;
    the lists [0, 2, 4] and [1, 5, 1] over a prefilled framebuffer are the masked oracle passes."""
    w, h, ts, pass_index = 96, 64, 32, 3
    s, d = MS.mixed_scene(ctl, w, h)
    p = ctl.PTParams(1, 12, 3, 1, ts, 1, 0, 0)
    pre = prefill(w, h, seed=7)
    snaps, _ = snapshots(orc, d, p, pass_index, pre, 2)
    assert not MS.same(snaps[1], pre)
    tracer.upload_scene(d)
    tracer.params = p
    for blocks in ([0, 2, 4], [1, 5, 1]):
        fb = torch.from_numpy(pre).to(dev)
        tracer.generate_samples(pass_index)
        tracer.render_pass_blocks(fb.data_ptr(), blocks)
        tracer.sync()
        exact(fb.cpu().numpy(), masked(snaps, blocks, w, h, ts), w)


def wpt_gpu(ctl, dev, desc, direct, shadow_any_hit=False):
    wt = ctl.WavefrontPathTracer(0, direct=direct, max_path_length=12, rr_start_depth=3, shadow_any_hit=shadow_any_hit)
    try:
        wt.upload_scene(desc)
        fb = torch.zeros((W * H, 7), dtype=torch.float32, device=dev)
        wt.reset_rays()
        for k in range(2):
            wt.do_pass(fb.data_ptr(), 1 + k, new_trace=(k == 0))
        torch.cuda.synchronize()
        return fb.cpu().numpy(), wt.rays_traced()
    finally:
        wt.close()


def wpt_oracle(orc, desc, direct):
    fb = np.zeros((W * H, 7), np.float32)
    rays = 0
    for k in range(2):
        rays += orc.oracle_wpt_render_pass(C.byref(desc), int(direct), 12, 3, k + 1, 1 + k, oracle.ptr(fb),
                                           tie_rule(desc, orc), 0)
    return fb, rays


@pytest.mark.parametrize("name,direct,bvh,any_hit", [(s, d, b, False) for s in "AB" for d in (True, False)
                                                     for b in ("wide", "binary")] + [("B", True, "wide", True)])
def test_wavefront_path_tracer_equals_the_oracle(ctl, orc, dev, name, direct, bvh, any_hit):
    """The WavefrontPathTracer's own integrator: its specular bit in the packed payload, its RR rule
    and its emitter sampling, two passes from first_pass = 1."""
    d = select_bvh(MS.scene(name)[1], bvh)
    want, wrays = wpt_oracle(orc, d, direct)
    got, grays = wpt_gpu(ctl, dev, d, direct, any_hit)
    assert grays == wrays
    assert np.isfinite(got).all() and got[:, :3].max() > 0
    exact(got, want)


@pytest.mark.parametrize("mode", range(12))
@pytest.mark.parametrize("name", ["A", "B"])
def test_prim_tracer_equals_the_oracle(ctl, orc, dev, name, mode):
    """Draw modes 0-11 with the depth image (the first_non_delta modes are refused on these scenes:
    test_wpt_and_prim_run_the_mixed_scene)."""
    d = MS.scene(name)[1]
    pt = ctl.PrimTracer(0, draw_mode=mode)
    try:
        pt.upload_scene(d)
        fb = torch.full((W * H, 7), 7.0, dtype=torch.float32, device=dev)   # DoPass clears it
        depth = torch.zeros(W * H, dtype=torch.float32, device=dev)
        pt.reset_rays()
        pt.do_pass(fb.data_ptr(), 3, depth.data_ptr())
        pt.sync()
        got, gdepth, grays = fb.cpu().numpy(), depth.cpu().numpy(), pt.rays_traced()
    finally:
        pt.close()
    pp = ctl.PrimParams(mode, 7, 1.0, 100000.0, 0)
    want, wdepth = np.zeros((W * H, 7), np.float32), np.zeros(W * H, np.float32)
    wrays = orc.oracle_prim_pass(C.byref(d), C.byref(pp), 3, oracle.ptr(want), oracle.ptr(wdepth), tie_rule(d, orc), 0)
    assert grays == wrays
    exact(got, want)
    assert np.array_equal(gdepth.view(np.uint32), wdepth.view(np.uint32))
