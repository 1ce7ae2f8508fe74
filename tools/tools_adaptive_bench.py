"""Adaptive-sampling measurements (block-list passes and the variance block
sampler) on the benchmark scene (C3 at 1920x1080 by default), device events
around >= 20 warmed passes each; prints one JSON line (--out FILE also writes it).

  (a) ctl_render_pass of another build of the library (--parent-lib, e.g. the
      parent commit's libctl_trace.so) and of this one, alternated in one
      process, the parent repeated so its own spread is known: the default
      kernels must not pay for the ownership policy.
  (b) ctl_render_pass_blocks with every block listed, against (a): the cost of
      the tables and the per-block apron items.
  (c) a mixed pass (variance sampler after 10 passes, fractions 2 / 4) against
      (a), next to the share of blocks it renders.
  (d) the host round trip of one adaptive pass (block statistics read-back,
      ranking and next list, table upload), from a host clock around a
      synchronised loop; the block statistics kernel is timed next to it.
A figure that was not taken is reported as "not measured"."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bind(path, abi):
    """Another build of the library: the symbols it has, bound as _abi.load binds them."""
    lib = C.CDLL(path)
    for name, res, args in abi.SYMBOLS:
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    return lib


class FullPasses:
    """ctl_render_pass on a context of `lib`, through plain ctypes calls: the same
    host path for the other build and for this one."""

    def __init__(self, lib, desc, params):
        self.lib, self.params = lib, params
        self.ctx = lib.ctl_create(0)
        if not self.ctx:
            raise RuntimeError("ctl_create failed on " + str(lib))
        self.check(lib.ctl_scene_upload(self.ctx, C.byref(desc)), "ctl_scene_upload")

    def check(self, status, what):
        if status != 0:
            raise RuntimeError(f"{what}: status {status}: " + (self.lib.ctl_last_error(self.ctx) or b"").decode())

    def call(self, fb_ptr):
        def one(k):
            self.check(self.lib.ctl_sampler_generate(self.ctx, 100 + k, 0), "ctl_sampler_generate")
            self.check(self.lib.ctl_render_pass(self.ctx, C.byref(self.params), fb_ptr, 0), "ctl_render_pass")
        return one

    def close(self):
        self.lib.ctl_destroy(self.ctx)
        self.ctx = None


def timed(torch, n, call):
    """ms per call over n calls between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(n):
        call(k)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--tile-size", type=int, default=64)
    ap.add_argument("--passes", type=int, default=24, help="timed passes per figure (>= 20)")
    ap.add_argument("--rounds", type=int, default=3, help="(a): parent / branch alternations")
    ap.add_argument("--parent-lib", default=None, help="libctl_trace.so of the build to compare (a) against")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench
    import cudatracerlib_amd as ctl
    from cudatracerlib_amd import _abi

    ba = bench.parse(["--config", str(a.config), "--scale", str(a.scale), "--width", str(a.width), "--height",
                      str(a.height)])
    owner, desc, source = bench.kept_scene(ctl, ba, bench.scene_threads())
    W, H, ts, n = a.width, a.height, a.tile_size, max(20, a.passes)
    dev = torch.device("cuda:0")
    fb = torch.zeros((W * H, 7), dtype=torch.float32, device=dev)
    params = ctl.PTParams(1, 50, 5, 1, ts, 1, 0, 0)   # one launch per pass, no render-ahead window
    pt = ctl.PathTracer(0, tile_size=ts)
    pt.params = params
    pt.upload_scene(desc)
    rec = {"workload": f"config {a.config} scale {a.scale:g} at {W}x{H}, {ts}-pixel blocks, {n} passes per figure",
           "scene": source}

    branch = FullPasses(ctl.lib(), desc, params)
    for k in range(3):
        branch.call(fb.data_ptr())(k)
    torch.cuda.synchronize()

    # (a)
    if a.parent_lib:
        parent = FullPasses(bind(a.parent_lib, _abi), desc, params)
        for k in range(3):
            parent.call(fb.data_ptr())(k)
        torch.cuda.synchronize()
        p_ms, b_ms = [], []
        for _ in range(a.rounds):
            p_ms.append(timed(torch, n, parent.call(fb.data_ptr())))
            b_ms.append(timed(torch, n, branch.call(fb.data_ptr())))
        p_ms.append(timed(torch, n, parent.call(fb.data_ptr())))
        parent.close()
        rec["a_render_pass_ms"] = {"parent": [round(x, 4) for x in p_ms], "branch": [round(x, 4) for x in b_ms],
                                   "branch_inside_parent_spread": bool(min(p_ms) <= np.median(b_ms) <= max(p_ms))}
        base = float(np.median(b_ms))
    else:
        rec["a_render_pass_ms"] = "not measured (no --parent-lib)"
        base = timed(torch, n, branch.call(fb.data_ptr()))
    branch.close()
    rec["render_pass_ms"] = round(base, 4)

    # (b)
    sampler = ctl.BlockSampler(W, H, ts, "variance")
    nb = sampler.num_blocks
    every = np.arange(nb, dtype=np.uint32)

    def list_pass(blocks):
        def call(k):
            pt.generate_samples(100 + k)
            pt.render_pass_blocks(fb.data_ptr(), blocks)
        return call

    list_pass(every)(0)
    torch.cuda.synchronize()
    all_ms = timed(torch, n, list_pass(every))
    rec["b_all_blocks_ms"] = round(all_ms, 4)
    rec["b_all_blocks_over_render_pass"] = round(all_ms / base, 4)

    # (d) and the ranking for (c): adaptive passes from a zeroed image
    fb.zero_()
    var = torch.zeros((W * H, 11), dtype=torch.float32, device=dev)
    info = torch.empty(5 * nb, dtype=torch.int32, device=dev)
    host_ms, stats_ms = [], []
    probe = ctl.BlockSampler(W, H, ts, "variance")   # a second sampler, so the timed round trip leaves the loop's alone
    # The real table upload is queued inside ctl_render_pass_blocks; (d) times a copy of the
    # tables' size (OwnList: 4 words per block) from pinned memory in its place.
    h_tbl = torch.zeros(4 * nb, dtype=torch.int32).pin_memory()
    d_tbl = torch.empty(4 * nb, dtype=torch.int32, device=dev)
    for k in range(10 + n):
        pt.do_pass_adaptive(fb.data_ptr(), var.data_ptr(), sampler, k)
        # on the state the pass left: the statistics kernel, then the round trip alone
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pt.block_stats(var.data_ptr(), W, H, ts, info.data_ptr())
        pt.sync()
        t1 = time.perf_counter()
        rec_np = info.cpu().numpy().view(ctl.BLOCK_INFO_DTYPE)   # read back
        probe.add_pass(rec_np)                                   # ranking (the sort)
        nxt = probe.blocks()
        d_tbl.copy_(h_tbl, non_blocking=True)                    # table upload
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if k >= 10:
            stats_ms.append((t1 - t0) * 1e3)
            host_ms.append((t2 - t1) * 1e3)
        del nxt
    rec["d_host_round_trip_ms"] = {"median": round(float(np.median(host_ms)), 4), "min": round(min(host_ms), 4),
                                   "max": round(max(host_ms), 4),
                                   "what": "20 B/block read-back + add_pass (ranking) + next list + upload of 16 "
                                           "B/block from pinned memory, synchronised"}
    rec["d_block_stats_ms"] = {"median": round(float(np.median(stats_ms)), 4),
                               "what": "ctl_block_stats + sync, host clock; not part of the round trip"}

    # (c)
    mixed = sampler.blocks()
    assert mixed.size < 2 * nb and np.unique(mixed).size < nb, "the sampler should be past its uniform passes"
    list_pass(mixed)(0)
    torch.cuda.synchronize()
    mixed_ms = timed(torch, n, list_pass(mixed))
    rec["c_mixed_pass_ms"] = round(mixed_ms, 4)
    rec["c_mixed_over_render_pass"] = round(mixed_ms / base, 4)
    rec["c_blocks"] = {"total": int(nb), "listed": int(mixed.size), "distinct": int(np.unique(mixed).size),
                       "share_traced": round(np.unique(mixed).size / nb, 4),
                       "share_of_samples": round(mixed.size / nb, 4)}
    pt.sync()
    pt.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
