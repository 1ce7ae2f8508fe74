"""The adaptive pass loop on the GPU (PathTracer.do_pass_adaptive: sampler tables,
block-list pass, variance pass, block statistics, read-back, sampler.add_pass)
with the variance block sampler: the framebuffer after every pass equals the
masked oracle driven by the same lists, the variance buffer equals the oracle's
with the same counts.  The ranking itself is checked in test_block_sampler.py."""
import numpy as np
import pytest

import oracle
from adaptive_helpers import differing, masked, num_blocks, snapshots

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def test_adaptive_loop(ctl, orc):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda:0")
    w, h, ts, passes = 96, 64, 32, 14
    s = ctl.HostScene().generate(2, 0.25, w, h)
    d = s.compile()
    pt = ctl.PathTracer(0, tile_size=ts)
    pt.upload_scene(d)
    sampler = ctl.BlockSampler(w, h, ts, "variance")
    nb = num_blocks(w, h, ts)
    fb = torch.zeros((w * h, 7), dtype=torch.float32, device=dev)
    var = torch.zeros((w * h, 11), dtype=torch.float32, device=dev)
    want = np.zeros((w * h, 7), np.float32)
    var_o = np.zeros((w * h, 11), np.float32)
    rendered = np.zeros(nb, np.uint32)
    for k in range(passes):
        expect_list = sampler.blocks()
        blocks = pt.do_pass_adaptive(fb.data_ptr(), var.data_ptr(), sampler, k)
        assert np.array_equal(blocks, expect_list)
        counts = np.bincount(blocks, minlength=nb).astype(np.uint8)
        rendered += counts
        if k < 10:
            assert np.array_equal(blocks, np.arange(nb))            # uniform until 10 passes are done
        else:
            assert np.unique(blocks).size < nb, (k, blocks)         # passes 11-14: fewer than all blocks
            assert blocks.size == nb // 4 + nb // 2
        snaps, _ = snapshots(orc, d, pt.params, k, want, int(counts.max()))
        want = masked(snaps, blocks, w, h, ts)
        got = fb.cpu().numpy()
        bad = differing(got, want)
        assert bad.size == 0, (k, blocks, bad[:10], want[bad[:3]], got[bad[:3]])
        orc.oracle_variance_add_pass(oracle.ptr(want), w, h, np.float32(1.0 / (k + 1)), ts, oracle.ptr(counts),
                                     oracle.ptr(var_o))
        assert np.array_equal(var.cpu().numpy().view(np.uint32), var_o.view(np.uint32)), k
        assert np.array_equal(sampler.passes_done(), rendered)
    pt.sync()
    sampler.close()
    pt.close()
