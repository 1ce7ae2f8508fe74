"""Cost of the kShadeSensors level: the generated scene C2 (--scale of its triangle budget) at 1920 x 1080
(a) under the perspective sensor, which runs the level the scene runs without a sensor record, and (b) under
a thin lens with aperture_radius = 0, which runs kShadeSensors on rays that differ from the pinhole's only by
roundings: one workload on two sets of kernels.  PathTracer, Direct = 1, MaxPathLength 50, RRStartDepth 5,
any-hit shadow rays, 64 passes in one ctl_render_passes launch (a window of about a tenth of a second), device
events around the launch, five launches each, alternating.  Prints one JSON line; it sets no threshold."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cudatracerlib_amd as ctl  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    args = ap.parse_args()
    w, h, passes, rounds = 1920, 1080, 64, 5
    hs = ctl.HostScene().generate(2, args.scale, w, h)
    desc = hs.compile()
    legs = {}
    for name in ("perspective", "thinlens_r0"):
        if name == "thinlens_r0":
            hs.set_sensor("thinlens", aperture_radius=0.0, focus_distance=10.0)   # refreshes desc in place
        pt = ctl.PathTracer(0)
        pt.upload_scene(desc)
        fb = torch.zeros((w * h, 7), dtype=torch.float32, device="cuda:0")
        pt.render_passes(fb.data_ptr(), 0, 2)   # warm-up
        torch.cuda.synchronize()
        legs[name] = (pt, fb, [], [])
    for r in range(rounds):
        for name, (pt, fb, rates, mss) in legs.items():
            pt.reset_rays()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            pt.render_passes(fb.data_ptr(), 2 + r * passes, passes)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
            mss.append(ms / passes)
            rates.append(pt.rays_traced() / (ms * 1e-3) / 1e6)
    out = {"scene": f"generate(2, {args.scale})", "triangles": int(desc.n_tri_data), "width": w, "height": h,
           "passes_per_launch": passes}
    for name, (pt, fb, rates, mss) in legs.items():
        pt.close()
        out[name] = {"mrays_s": [round(x, 1) for x in rates], "median_mrays_s": round(sorted(rates)[rounds // 2], 1),
                     "median_ms_per_pass": round(sorted(mss)[rounds // 2], 4)}
    out["ratio_sensors_over_perspective"] = round(out["thinlens_r0"]["median_mrays_s"] / out["perspective"]["median_mrays_s"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
