"""ctl_render_pass_blocks on the GPU, bit for bit against the masked oracle
(adaptive_helpers): a block-list pass is a full pass masked to the listed
blocks, m times in succession for a block listed m times.  Also the per-block
statistics (ctl_block_stats) and every refusal."""
import ctypes as C

import numpy as np
import pytest

import oracle
from adaptive_helpers import block_of_pixel, differing, masked, num_blocks, prefill, snapshots
from helpers import alpha_scene, binary_bvh, jitter_landing, select_bvh

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TS = 32


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


SCENES = {}


def scene(ctl, config, scale, w, h):
    key = (config, scale, w, h)
    if key not in SCENES:
        s = ctl.HostScene().generate(config, scale, w, h)
        SCENES[key] = (s, s.compile())
    return SCENES[key][1]


def render_list(tracer, dev, params, pass_index, pre, lists, generate=True):
    """The framebuffer after the block lists `lists` (one call each, same tables) over `pre`."""
    tracer.params = params
    fb = torch.from_numpy(pre).to(dev)
    if generate:
        tracer.generate_samples(pass_index)
    for blocks in lists:
        tracer.render_pass_blocks(fb.data_ptr(), blocks)
    tracer.sync()                                  # ctl_sync is clean after each case
    return fb.cpu().numpy()


def check(got, want, what):
    bad = differing(got, want)
    assert bad.size == 0, (what, bad[:10], want[bad[:3]], got[bad[:3]])


@pytest.mark.parametrize("w,h", [(96, 64), (72, 40)])           # 3 x 2 blocks; partial edge blocks
@pytest.mark.parametrize("bvh", ["wide", "binary"])
@pytest.mark.parametrize("direct", [1, 0])
def test_block_lists_bit_exact(ctl, orc, tracer, dev, w, h, bvh, direct):
    d = select_bvh(scene(ctl, 2, 0.25, w, h), bvh)
    p = ctl.PTParams(direct, 50, 5, 1, TS, 1, 0, 0)
    nb = num_blocks(w, h, TS)
    assert nb == 6
    pass_index = 3
    pre = prefill(w, h, seed=w + direct)
    snaps, orays = snapshots(orc, d, p, pass_index, pre, 3)
    assert differing(snaps[1], pre).size == w * h               # the pass touches every pixel
    tracer.upload_scene(d)
    every = np.arange(nb, dtype=np.uint32)
    cases = {"one block": [4], "checkerboard": [0, 2, 4], "twice": [1, 5, 1], "three times": [3, 0, 3, 3],
             "all blocks": every}
    for what, blocks in cases.items():
        got = render_list(tracer, dev, p, pass_index, pre, [blocks])
        check(got, masked(snaps, blocks, w, h, TS), what)
    # all blocks: ctl_render_pass itself, with the oracle's ray count
    tracer.reset_rays()
    got = render_list(tracer, dev, p, pass_index, pre, [every])
    assert tracer.rays_traced() == orays
    fb = torch.from_numpy(pre).to(dev)
    tracer.render_pass(fb.data_ptr())
    tracer.sync()
    check(got, fb.cpu().numpy(), "all blocks against ctl_render_pass")
    check(got, snaps[1], "all blocks against the full oracle pass")
    # two disjoint lists one after the other on the same tables: the full pass
    got = render_list(tracer, dev, p, pass_index, pre, [[5, 0, 3], [2, 4, 1]])
    check(got, snaps[1], "two disjoint lists")
    # four queued without a sync between them: each table staging half is reused once
    got = render_list(tracer, dev, p, pass_index, pre, [[5], [0, 3], [2], [4, 1]])
    check(got, snaps[1], "four disjoint lists")
    assert tracer.last_pass_ms() > 0.0                           # ctl_last_pass_ms covers the call


STRAY_TS = 8


# 4096 x 8: one row of blocks, strays to the right (the left-column apron items).
# 8 x 4200: one column of blocks, strays downwards (the top-row apron items); with this
# repository's oracle on the CPU pass 10 has 2 and pass 17 has 2 that land in another block.
# 256 x 256: a 32 x 32 grid of blocks, so block ids and apron pixels go through tiles_x;
# pass 2 has 1 downwards and pass 14 has 1 to the right.
@pytest.mark.parametrize("w,h,pass_index", [(4096, 8, 7), (4096, 8, 18), (8, 4200, 10), (8, 4200, 17),
                                            (256, 256, 2), (256, 256, 14)])
def test_strays_across_blocks(ctl, orc, tracer, dev, w, h, pass_index):
    """Samples whose jitter carries them into another block (floor(x + u) one pixel on):
    summed by the block they land on -- traced through an apron item when their own block
    is not listed, dropped when they leave the list."""
    ts = STRAY_TS
    lx, ly = jitter_landing(orc, pass_index, w, h)
    blk = block_of_pixel(w, h, ts)
    inside = (lx < w) & (ly < h)
    land = np.where(inside, (ly // ts) * (-(-w // ts)) + lx // ts, blk)
    strays = np.nonzero(land != blk)[0]
    assert strays.size >= 1, "the shape was chosen to have samples that land in another block"
    d = scene(ctl, 2, 0.05, w, h)
    p = ctl.PTParams(1, 50, 5, 1, ts, 1, 0, 0)
    nb = num_blocks(w, h, ts)
    pre = prefill(w, h, seed=pass_index)
    snaps, _ = snapshots(orc, d, p, pass_index, pre, 1)
    tracer.upload_scene(d)
    tracer.params = p
    tracer.generate_samples(pass_index)
    every = np.arange(nb, dtype=np.uint32)
    for s in strays:
        a, b = int(blk[s]), int(land[s])
        for what, blocks in [("all but a", every[every != a]), ("all but b", every[every != b]), ("only a", [a]),
                             ("only b", [b])]:
            got = render_list(tracer, dev, p, pass_index, pre, [blocks], generate=False)
            check(got, masked(snaps, blocks, w, h, ts), (what, a, b))


def c5_scene(ctl):
    return scene(ctl, 5, 0.003, 96, 64)                          # C5 materials: the FULL kernel


def env_scene_96(ctl):
    if "env" not in SCENES:
        from test_env_light import env_scene
        SCENES["env"] = env_scene(ctl, textured=True, w=96, h=64)   # environment map: the env kernel
    return SCENES["env"][1]


# c5, env, alpha: the shading levels above lean (materials_oracle's block-list test runs the
# mat level); two-level: the Cornell box, one node per shape, in the reference's binary order
@pytest.mark.parametrize("which", ["c5", "env", "alpha", "two-level"])
def test_full_shading_kernels(ctl, orc, tracer, dev, which):
    d = {"c5": c5_scene, "env": env_scene_96, "alpha": lambda c: alpha_scene(c)[0],
         "two-level": lambda c: binary_bvh(scene(c, 1, 1.0, 96, 64))}[which](ctl)
    assert (d.scene_start_node >= 0) == (which == "two-level")
    p = ctl.PTParams(1, 8, 3, 1, TS, 1, 0, 0)
    pre = prefill(96, 64, seed=11)
    snaps, _ = snapshots(orc, d, p, 2, pre, 1)
    assert differing(snaps[1], pre).size > 96 * 64 // 2
    tracer.upload_scene(d)
    blocks = [0, 2, 4]
    check(render_list(tracer, dev, p, 2, pre, [blocks]), masked(snaps, blocks, 96, 64, TS), which)


def test_refusals(ctl, orc, tracer, dev):
    w, h = 96, 64
    d = scene(ctl, 2, 0.25, w, h)
    tracer.upload_scene(d)
    pre = prefill(w, h, seed=1)
    fb = torch.from_numpy(pre).to(dev)
    tracer.generate_samples(0)

    def refused(params, blocks, match):
        tracer.params = params
        with pytest.raises(ctl.CTLError, match=match):
            tracer.render_pass_blocks(fb.data_ptr(), blocks)

    ok = ctl.PTParams(1, 50, 5, 1, TS, 1, 0, 0)
    refused(ctl.PTParams(1, 50, 5, 1, TS, 2, 0, 0), [0], "num_ranks")
    refused(ctl.PTParams(1, 50, 5, 1, TS, 1, 0, ctl.CTL_PT_MEGAKERNEL), [0], "CTL_PT_MEGAKERNEL")
    refused(ctl.PTParams(1, 50, 5, 1, TS, 1, 0, ctl.CTL_PT_WAVEFRONT), [0], "CTL_PT_WAVEFRONT")
    refused(ok, [0, 6], "block id 6")                            # 6 blocks: ids 0..5
    refused(ok, [2] * 256, "255")
    tracer.params = ok
    tracer.render_pass_blocks(fb.data_ptr(), [2] * 255)          # the uint8 flag's range
    tracer.sync()
    snaps, _ = snapshots(orc, d, ok, 0, pre, 1)
    one = snaps[1] - pre                                         # not used for bits: only that block 2 moved
    got = fb.cpu().numpy()
    moved = differing(got, pre)
    assert moved.size and np.all(block_of_pixel(w, h, TS)[moved] == 2) and np.abs(one).max() > 0
    # n_blocks == 0: CTL_OK, nothing written
    fb2 = torch.from_numpy(pre).to(dev)
    tracer.render_pass_blocks(fb2.data_ptr(), [])
    tracer.sync()
    assert differing(fb2.cpu().numpy(), pre).size == 0
    assert ctl.lib().ctl_render_pass_blocks(tracer._ctx, C.byref(ok), None, 3, fb2.data_ptr(), None) != 0


def test_render_ahead_flag_ignored_and_window_dropped(ctl, orc, tracer, dev):
    """CTL_PT_RENDER_AHEAD does not change a block-list pass, and a window that
    ctl_render_pass rendered ahead is dropped by it: the next do_pass renders afresh."""
    w, h = 96, 64
    d = scene(ctl, 2, 0.25, w, h)
    p = ctl.PTParams(1, 50, 5, 1, TS, 1, 0, ctl.CTL_PT_RENDER_AHEAD)
    tracer.upload_scene(d)
    tracer.params = p
    fb = torch.zeros((w * h, 7), dtype=torch.float32, device=dev)
    want = np.zeros((w * h, 7), np.float32)
    for k in (0, 1):                                             # the second call renders pass 2 ahead
        tracer.do_pass(fb.data_ptr(), k)
        want = snapshots(orc, d, p, k, want, 1)[0][1]
    tracer.generate_samples(9)
    tracer.render_pass_blocks(fb.data_ptr(), [1, 4])
    want = masked(snapshots(orc, d, p, 9, want, 1)[0], [1, 4], w, h, TS)
    tracer.do_pass(fb.data_ptr(), 2)
    want = snapshots(orc, d, p, 2, want, 1)[0][1]
    tracer.sync()
    check(fb.cpu().numpy(), want, "passes 0, 1, a block list on pass 9's tables, pass 2")


# ---- ctl_block_stats -------------------------------------------------------


@pytest.fixture(scope="module")
def variance_buffers(ctl, dev):
    """Variance buffers after 3 uniform passes at 96x64 and 72x40, computed once."""
    out = {}
    pt = ctl.PathTracer(0, tile_size=TS)
    for w, h in [(96, 64), (72, 40)]:
        pt.upload_scene(scene(ctl, 2, 0.25, w, h))
        fb = torch.zeros((w * h, 7), dtype=torch.float32, device=dev)
        var = torch.zeros((w * h, 11), dtype=torch.float32, device=dev)
        for k in range(3):
            pt.do_pass(fb.data_ptr(), k)
            pt.variance_add_pass(fb.data_ptr(), w, h, np.ones(num_blocks(w, h, TS), np.uint8), var.data_ptr(),
                                 splat_scale=1.0 / (k + 1), tile_size=TS)
        pt.sync()
        out[(w, h)] = var
    yield pt, out
    pt.close()


def block_stats(ctl, pt, dev, var, w, h):
    n = num_blocks(w, h, TS)
    out = torch.full((n, 5), -1, dtype=torch.int32, device=dev)
    pt.block_stats(var.data_ptr(), w, h, TS, out.data_ptr())
    pt.sync()
    return out.cpu().numpy().reshape(-1).view(ctl.BLOCK_INFO_DTYPE)


@pytest.mark.parametrize("w,h", [(96, 64), (72, 40)])
def test_block_stats(ctl, dev, variance_buffers, w, h):
    pt, bufs = variance_buffers
    var = bufs[(w, h)]
    got = block_stats(ctl, pt, dev, var, w, h)
    again = block_stats(ctl, pt, dev, var, w, h)
    assert got.tobytes() == again.tobytes()                      # two calls: identical bytes
    stats = torch.zeros((2, w * h), dtype=torch.float32, device=dev)
    pt.variance_stats(var.data_ptr(), w * h, None, stats[0].data_ptr(), stats[1].data_ptr())
    pt.sync()
    variance, e = stats.cpu().numpy()
    e2 = e * e                                                   # squared in fp32
    blk = block_of_pixel(w, h, TS)
    bound = TS * TS * 2.0 ** -24        # worst case of any fp32 summation order over n non-negative terms
    for b in range(num_blocks(w, h, TS)):
        m = blk == b
        ok = m & (variance >= 0) & ~np.isnan(variance)
        assert got["num_pixels_e"][b] == m.sum()
        assert got["num_pixels_var"][b] == ok.sum() > 0
        for name, terms in [("block_var_i", variance[ok]), ("block_e_i", e[m]), ("block_e_i2", e2[m])]:
            want = terms.astype(np.float64).sum()
            assert np.all(terms >= 0) and want > 0
            rel = abs(float(got[name][b]) - want) / want
            print(f"{w}x{h} block {b} {name}: relative difference {rel:.3e} (bound {bound:.3e})")
            assert rel <= bound, (name, b, rel)


def test_block_stats_zeroed_record(ctl, dev, variance_buffers):
    """A pixel without a variance sample (a record zeroed by hand): e = 0 / 0, so the
    block's e sums are NaN as in the reference, and its variance stays out of the sums."""
    pt, bufs = variance_buffers
    w, h = 96, 64
    var = bufs[(w, h)].clone()
    base = block_stats(ctl, pt, dev, var, w, h)
    x, y = 40, 37                                                # block 4
    var[y * w + x] = 0
    got = block_stats(ctl, pt, dev, var, w, h)
    assert np.isnan(got["block_e_i"][4]) and np.isnan(got["block_e_i2"][4])
    assert got["num_pixels_e"][4] == base["num_pixels_e"][4]
    assert got["num_pixels_var"][4] == base["num_pixels_var"][4] - 1
    assert got["block_var_i"][4] <= base["block_var_i"][4] and np.isfinite(got["block_var_i"][4])
    others = np.arange(6) != 4
    assert got[others].tobytes() == base[others].tobytes()
