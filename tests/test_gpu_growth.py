"""One context taken through growing and shrinking work: every buffer that a
context grows on demand (sample slots, sampler tables of a multi-pass launch,
block tables, wavefront and WavefrontPathTracer queues, block flags, the image
pipeline's scratch) is exercised at 16x16 (1 tile of 64), then 72x40 (2 tiles),
then 16x16 again, and every result must equal, bit for bit, the same call on a
fresh context created at that size."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIZES = [(16, 16), (72, 40), (16, 16)]


def run_all(ctl, pt, dev, w, h):
    """Every growth path once at w x h; the results by name."""
    abi = ctl._abi
    s = ctl.HostScene().generate(2, 0.05, w, h)
    pt.upload_scene(s.compile())
    n = w * h
    tiles = ((w + 63) // 64) * ((h + 63) // 64)
    out = {}

    def fresh_fb():
        return torch.zeros((n, 7), dtype=torch.float32, device=dev)

    for name, flag in (("persistent", 0), ("megakernel", ctl.CTL_PT_MEGAKERNEL), ("wavefront", ctl.CTL_PT_WAVEFRONT)):
        pt.params.flags = flag
        fb = fresh_fb()
        pt.do_pass(fb.data_ptr(), 0)
        out[name] = fb
    pt.params.flags = 0
    fb = fresh_fb()
    pt.render_passes(fb.data_ptr(), 1, 2)
    out["render_passes"] = fb
    fb = fresh_fb()
    pt.generate_samples(3)
    pt.render_pass_blocks(fb.data_ptr(), list(range(tiles)) + [0])          # block 0 twice
    out["blocks"] = fb
    fb = fresh_fb()
    wp = ctl.WptParams(1, 50, 5, 1, 0)
    pt.generate_samples(4)
    ctl._check(pt._L.ctl_wpt_render_pass(pt._ctx, C.byref(wp), fb.data_ptr(), 0), pt._ctx, "ctl_wpt_render_pass")
    out["wpt"] = fb
    var = torch.zeros((n, 11), dtype=torch.float32, device=dev)
    pt.variance_add_pass(out["render_passes"].data_ptr(), w, h, np.ones(tiles, np.uint8), var.data_ptr(),
                         splat_scale=0.5)
    out["variance"] = var
    rgba = torch.zeros(n, dtype=torch.int32, device=dev)
    pt.image_pipeline(out["render_passes"].data_ptr(), w, h, rgba.data_ptr(), filter=ctl.image_filter(abi.CTL_FILTER_NLM),
                      var_ptr=var.data_ptr(), splat_scale=0.5, num_passes=2)
    out["nlm"] = rgba
    pt.sync()
    res = {k: v.cpu().numpy().view(np.uint32) for k, v in out.items()}
    res["rays_traced"] = pt.rays_traced()
    pt.reset_rays()
    return res


def test_growth_matches_fresh_contexts(ctl):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda:0")
    want = {}
    for w, h in sorted(set(SIZES)):
        pt = ctl.PathTracer(0)
        want[(w, h)] = run_all(ctl, pt, dev, w, h)
        pt.close()
    pt = ctl.PathTracer(0)
    for step, (w, h) in enumerate(SIZES):
        got = run_all(ctl, pt, dev, w, h)
        ref = want[(w, h)]
        assert got.keys() == ref.keys()
        for k in ref:
            if k == "rays_traced":
                assert got[k] == ref[k] and got[k] > 0, (step, w, h, got[k], ref[k])
            else:
                assert np.array_equal(got[k], ref[k]), (step, w, h, k)
        assert np.any(ref["persistent"]) and np.any(ref["wpt"]) and np.any(ref["nlm"])
    pt.close()
