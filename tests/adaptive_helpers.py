"""The masked oracle of a block-list pass (ctl_render_pass_blocks), shared by
test_gpu_block_pass.py and test_gpu_adaptive.py (test infrastructure).

A block-list pass is a full pass masked to the listed blocks: the expected
framebuffer takes, for a pixel of a block listed m times, the framebuffer after
m full oracle passes (same pass index) over the pre-filled framebuffer, and the
pre-filled bytes everywhere else."""
import ctypes as C

import numpy as np

import oracle
from helpers import tie_rule


def prefill(w, h, seed):
    """A framebuffer of random finite floats (PixelData rows)."""
    rng = np.random.default_rng(seed)
    return (rng.random((w * h, 7), dtype=np.float32) * np.float32(4.0)).astype(np.float32)


def block_of_pixel(w, h, ts):
    idx = np.arange(w * h, dtype=np.int64)
    return ((idx // w) // ts) * (-(-w // ts)) + (idx % w) // ts


def num_blocks(w, h, ts):
    return (-(-w // ts)) * (-(-h // ts))


def snapshots(orc, desc, params, pass_index, pre, m):
    """[pre, pre + 1 full pass, ..., pre + m full passes] and the rays of one pass."""
    snaps = [pre.copy()]
    fb = pre.copy()
    rays = 0
    for _ in range(m):
        rays = orc.oracle_render_pass(C.byref(desc), C.byref(params), pass_index, oracle.ptr(fb), tie_rule(desc, orc),
                                      0, 1, None)
        snaps.append(fb.copy())
    return snaps, rays


def masked(snaps, blocks, w, h, ts):
    """The expected framebuffer of one block-list pass over snaps[0]."""
    counts = np.bincount(np.asarray(blocks, np.int64), minlength=num_blocks(w, h, ts))
    assert counts.max(initial=0) < len(snaps)
    m = counts[block_of_pixel(w, h, ts)]
    stack = np.stack(snaps)                       # (m + 1, pixels, 7)
    return stack[m, np.arange(w * h)]


def differing(a, b):
    return np.nonzero((a.view(np.uint32) != b.view(np.uint32)).any(axis=1))[0]
