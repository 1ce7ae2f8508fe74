"""Throughput of the mixed-material test scene (tests/materials_scenes.py::mixed_scene: a diffuse
floor, an area light, an environment map and one card each of dielectric, thindielectric, conductor,
roughconductor and plastic) at 1920 x 1080: PathTracer, Direct = 1, MaxPathLength 50, RRStartDepth 5,
any-hit shadow rays, passes in one ctl_render_passes launch, device events around the launch.
Prints one JSON line.  A first number for the kShadeMat kernels, not a benchmark of the project."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cudatracerlib_amd as ctl  # noqa: E402
from materials_scenes import mixed_scene  # noqa: E402


def main():
    w, h, passes, rounds = 1920, 1080, 16, 5
    hs, d = mixed_scene(ctl, w, h)
    pt = ctl.PathTracer(0)
    pt.upload_scene(d)
    fb = torch.zeros((w * h, 7), dtype=torch.float32, device="cuda:0")
    pt.render_passes(fb.data_ptr(), 0, 4)   # warm-up
    torch.cuda.synchronize()
    rates = []
    for r in range(rounds):
        pt.reset_rays()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        pt.render_passes(fb.data_ptr(), 4 + r * passes, passes)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        rates.append(pt.rays_traced() / (ms * 1e-3) / 1e6)
    pt.close()
    print(json.dumps({"scene": "mixed materials, 24 triangles", "width": w, "height": h, "passes_per_launch": passes,
                      "mrays_s": [round(x, 1) for x in rates], "median_mrays_s": round(sorted(rates)[len(rates) // 2], 1)}))


if __name__ == "__main__":
    main()
