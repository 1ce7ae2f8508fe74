"""Deepest traversal stack the oracle's three visit orders reach on the unit-test
scenes ("The traversal stack"): 50 000 random rays, the 96 x 64
camera rays and two render passes per scene, the inputs of tests/test_gpu_parity.py.
Sizes include the sentinel.  CPU only.  usage: python tools/stack_depth.py [--large]"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import cudatracerlib_amd as ctl  # noqa: E402
import oracle  # noqa: E402
from helpers import camera_rays, oracle_render, random_rays, select_bvh, tie_rule  # noqa: E402


def main():
    orc = oracle.load()
    scenes = [(1, 1.0), (2, 0.25), (3, 0.004), (5, 0.003)] + ([(3, 0.05)] if "--large" in sys.argv else [])
    print("| scene | triangles | upload bound (binary, wide) | deepest stack reached: wide / wideq / binary |")
    print("|---|---|---|---|")
    for config, scale in scenes:
        hs = ctl.HostScene().generate(config, scale, 96, 64)
        d0 = hs.compile()
        mesh = [ctl.bvh_stack_bound(C.cast(C.addressof(d0.bvh_nodes.contents) + 64 * (d0.meshes[m].bvh_node_offset // 4),
                                           C.POINTER(ctl._abi.BVHNode * (d0.n_bvh_nodes - d0.meshes[m].bvh_node_offset // 4))
                                           ).contents) for m in range(d0.n_meshes)]
        b, w = max(x[0] for x in mesh), max(x[1] for x in mesh)
        if d0.scene_start_node >= 0:
            top = ctl.bvh_stack_bound(C.cast(d0.scene_bvh_nodes, C.POINTER(ctl._abi.BVHNode * d0.n_scene_bvh_nodes)).contents,
                                      d0.scene_start_node)
            b, w = top[0] + 1 + b, top[1] + 1 + w
        peaks = []
        for bvh in ("wide", "wideq", "binary"):
            d = select_bvh(d0, bvh)
            orc.oracle_depth_peak_reset()
            for rays in (random_rays(d, 50000, seed=config), camera_rays(d, 96, 64, seed=config)):
                n = rays.shape[0]
                hits, depth = np.zeros((n, 4), np.int32), np.zeros(n, np.int32)
                orc.oracle_intersect_depth(C.byref(d), n, oracle.ptr(rays), oracle.ptr(hits), 0, tie_rule(d, orc), 0,
                                           oracle.ptr(depth))
            oracle_render(orc, d, ctl.PTParams(1, 50, 5, 1, 64, 1, 0, 0), 2, 96, 64)
            peaks.append(orc.oracle_depth_peak())
        print("| C%d %g | %d | %d, %d | %d / %d / %d |" % (config, scale, d0.n_tri_data, b, w, *peaks))


if __name__ == "__main__":
    main()
