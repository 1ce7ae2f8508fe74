"""Image-pipeline stage timings (ctl_image_pipeline, ctl_image_luminance) at
1920x1080 by default, on the framebuffer and the variance buffer of a few
passes of the C2 scene.  Each stage is timed with device events around one
call: warm-up calls first, then the median (and min / max) of repeated calls.
Prints one JSON line; --out FILE also writes it (profiles/image_pipeline.json).

Stages: each canonical filter at the reference's default widths (the Gaussian
with alpha 2: the reference's default alpha, -2, makes every weight 0); the
non-local-means filter recomputing its weights and applying them, as the
reference structures it (CTL_NLM_DIRECT) and with the shared tap terms (the
default), both fused (update_periodicity 1, no weight buffer) and through the
weight buffer; apply-only with kept weights; the luminance reduction; the tone
map (process-only pipeline: copy to RGBE, luminance, Reinhard, gamma).
For the NLM stages the bytes moved are given next to the time: what the
kernels read and write in device memory, counted from the launch geometry."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--scale", type=float, default=0.05, help="C2 scene scale")
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="recorded as given (default: git rev-parse of this tree)")
    a = ap.parse_args()

    import torch
    import cudatracerlib_amd as ctl
    from cudatracerlib_amd import _abi

    w, h, n = a.width, a.height, a.width * a.height
    dev = torch.device("cuda:0")
    scene = ctl.HostScene().generate(2, a.scale, w, h)
    pt = ctl.PathTracer(0)
    pt.upload_scene(scene.compile())
    fb = torch.zeros((n, 7), dtype=torch.float32, device=dev)
    var = torch.zeros((n, 11), dtype=torch.float32, device=dev)
    tiles = ((w + 63) // 64) * ((h + 63) // 64)
    for p in range(a.passes):
        pt.do_pass(fb.data_ptr(), p)
        pt.variance_add_pass(fb.data_ptr(), w, h, np.ones(tiles, np.uint8), var.data_ptr())
    pt.sync()
    rgba = torch.zeros(n, dtype=torch.int32, device=dev)
    flt = torch.zeros(n, dtype=torch.int32, device=dev)

    def timed(call, reps=a.reps, warmup=a.warmup):
        for k in range(warmup):
            call(k)
        torch.cuda.synchronize()
        ms = []
        for k in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call(warmup + k)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                "reps": reps}

    def pipeline(filt=None, tonemap=None, passes=lambda k: 0):
        return lambda k: pt.image_pipeline(fb.data_ptr(), w, h, rgba.data_ptr(), filter=filt, tonemap=tonemap,
                                           var_ptr=var.data_ptr(), filtered_ptr=flt.data_ptr(), num_passes=passes(k))

    stages = {}
    stages["resolve"] = timed(pipeline())
    for name, t, kw in [("box", _abi.CTL_FILTER_BOX, {}), ("gaussian_alpha2", _abi.CTL_FILTER_GAUSSIAN, dict(a=2.0)),
                        ("mitchell", _abi.CTL_FILTER_MITCHELL, {}), ("lanczos", _abi.CTL_FILTER_LANCZOS, {}),
                        ("triangle", _abi.CTL_FILTER_TRIANGLE, {})]:
        stages["filter_" + name] = timed(pipeline(ctl.image_filter(t, **kw)))

    # bytes in device memory per NLM call: the tile loads (each workgroup reads its 34 x 34 halo of 28-B
    # pixels and, when it computes weights, of the 12 B of the 44-B variance records it uses), the filtered
    # image written, the RGBE read and RGBA written by copyFilteredToOutput, and the weight buffer
    tiles16 = ((w + 15) // 16) * ((h + 15) // 16)
    halo_px = tiles16 * 34 * 34
    out_bytes = 3 * 4 * n
    wbytes = 169 * 4 * n
    nlm_bytes = {"fused": halo_px * (28 + 12) + out_bytes, "store": halo_px * (28 + 12) + out_bytes + wbytes,
                 "apply": halo_px * 28 + out_bytes + wbytes}
    nlm = {}
    # the two variants alternated so drift hits both alike
    for rnd in range(2):
        for variant, flags in [("direct", _abi.CTL_NLM_DIRECT), ("shared", 0)]:
            r = timed(pipeline(ctl.image_filter(_abi.CTL_FILTER_NLM, update_periodicity=1, flags=flags)),
                      reps=max(3, a.reps // 2), warmup=1)
            nlm.setdefault("nlm_%s_fused" % variant, []).append(r)
            # every call a jump in num_passes: recompute into the weight buffer, then apply
            r = timed(pipeline(ctl.image_filter(_abi.CTL_FILTER_NLM, update_periodicity=25, flags=flags),
                               passes=lambda k: 2 * k + 1), reps=max(3, a.reps // 2), warmup=1)
            nlm.setdefault("nlm_%s_store" % variant, []).append(r)
    for key, runs in nlm.items():
        best = min(runs, key=lambda r: r["median_ms"])
        stages[key] = dict(best, runs_median_ms=[r["median_ms"] for r in runs],
                           bytes_moved=nlm_bytes["fused" if key.endswith("fused") else "store"])
    # apply-only: consecutive passes that never hit the periodicity
    f25 = ctl.image_filter(_abi.CTL_FILTER_NLM, update_periodicity=1 << 30)
    pipeline(f25, passes=lambda k: 5)(0)
    stages["nlm_apply_only"] = dict(timed(pipeline(f25, passes=lambda k: 6 + k), warmup=2), bytes_moved=nlm_bytes["apply"])

    stages["luminance"] = timed(lambda k: pt.image_luminance(flt.data_ptr(), w, h))
    stages["tonemap_pipeline"] = timed(pipeline(tonemap=ctl.Tonemap(0.18, 0.0)))
    stages["to_filtered_plus_output"] = timed(pipeline(ctl.image_filter(_abi.CTL_FILTER_BOX, 0.5, 0.5)))

    try:
        if a.commit:
            raise LookupError
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                                check=True).stdout.strip()
        dirty = bool(subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "-uno"], capture_output=True,
                                    text=True).stdout.strip())
    except Exception:
        commit, dirty = a.commit or "unknown", False
    d, s = stages["nlm_direct_fused"]["median_ms"], stages["nlm_shared_fused"]["median_ms"]
    res = {"tool": "tools/image_pipeline_bench.py", "commit": commit + ("+changes" if dirty else ""),
           "device": torch.cuda.get_device_name(0), "width": w, "height": h, "passes": a.passes, "scene": "C2",
           "timing": "device events around one call; median of reps after warm-up", "stages": stages,
           "nlm_speedup_shared_over_direct": round(d / s, 3) if s > 0 else None,
           "nlm_default": "shared" if s <= d else "direct"}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    pt.close()


if __name__ == "__main__":
    main()
