"""Cost of the kShadeMedia level: the fog room of tests/media_cases.py::fog_room at 1920 x 1080 (a closed
room of 16 triangles, an area light and a point light) (a) without the volume, which runs the
kShadeLights kernels, and (b) with a coloured Henyey-Greenstein fog over room and camera, which runs
kShadeMedia.  PathTracer, Direct = 1, MaxPathLength 50, RRStartDepth 5, any-hit shadow rays, 16 passes in
one ctl_render_passes launch, device events around the launch, five launches each, alternating.
Prints one JSON line.  The two legs do not shade the same paths (in the fog most events are medium
interactions, which trace a ray and shade no surface), so the rates compare two workloads, not two
kernels on one; it sets no threshold."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cudatracerlib_amd as ctl  # noqa: E402
from media_cases import fog_room  # noqa: E402


def main():
    w, h, passes, rounds = 1920, 1080, 16, 5
    legs = {}
    for name, fog in (("clear_room", False), ("fog_room", True)):
        hs = fog_room(ctl, fog, w, h)
        pt = ctl.PathTracer(0)
        pt.upload_scene(hs.compile())
        fb = torch.zeros((w * h, 7), dtype=torch.float32, device="cuda:0")
        pt.render_passes(fb.data_ptr(), 0, 4)   # warm-up
        torch.cuda.synchronize()
        legs[name] = (hs, pt, fb, [], [])
    for r in range(rounds):
        for name, (hs, pt, fb, rates, mss) in legs.items():
            pt.reset_rays()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            pt.render_passes(fb.data_ptr(), 4 + r * passes, passes)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
            mss.append(ms / passes)
            rates.append(pt.rays_traced() / (ms * 1e-3) / 1e6)
    out = {"scene": "media_cases.fog_room, 16 triangles", "width": w, "height": h, "passes_per_launch": passes}
    for name, (hs, pt, fb, rates, mss) in legs.items():
        pt.close()
        out[name] = {"mrays_s": [round(x, 1) for x in rates], "median_mrays_s": round(sorted(rates)[rounds // 2], 1),
                     "median_ms_per_pass": round(sorted(mss)[rounds // 2], 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
