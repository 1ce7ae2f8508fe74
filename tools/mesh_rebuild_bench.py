"""ctl_scene_rebuild_mesh timings: milliseconds per rebuild (device events around
the call: the median of --reps after --warmup), the host time of its two stream
synchronisations (ctl_last_rebuild_ms), and the camera-ray ctl_intersect rate on
the rebuilt LBVH trees against the same mesh's uploaded SBVH trees, in one
process.  Two meshes: the 2 M-triangle grid of bench.py's animation leg
(tools/tools_anim_bench.py, here a static mesh), and the largest mesh of
bench.py's default scene (C3), taken from the kept scene cache when it is there
(else compiled, and the compile seconds are reported).  The C3 positions are
recovered from the compiled Woop records (the desc keeps no vertices), so they
equal the compiled ones up to fp32 rounding; a triangle the compile dropped as
degenerate gets three equal vertices.
Prints one JSON line; --out FILE also writes it (profiles/mesh_rebuild.json)."""
import argparse
import hashlib
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_module(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def positions_from_woop(desc, mesh):
    """(n, 9) float32 positions of mesh `mesh` from its Woop records: the record is rows 2, 0, 1
    of the inverse of [v0 - v2, v1 - v2, n, v2]."""
    import ctypes as C
    M = desc.meshes[mesh]
    offs = sorted(desc.meshes[i].triangle_offset for i in range(desc.n_meshes)) + [desc.n_tri_data]
    n = offs[offs.index(M.triangle_offset) + 1] - M.triangle_offset
    eoffs = sorted(desc.meshes[i].bvh_indices_offset for i in range(desc.n_meshes)) + [desc.n_tri_indices]
    e0 = M.bvh_indices_offset
    e1 = eoffs[eoffs.index(e0) + 1]
    idx = np.ctypeslib.as_array(C.cast(desc.tri_indices, C.POINTER(C.c_uint32)), shape=(desc.n_tri_indices,))[e0:e1] >> 1
    woop = np.ctypeslib.as_array(C.cast(desc.woop_tris, C.POINTER(C.c_float)), shape=(desc.n_woop_tris * 12,))
    woop = woop.reshape(-1, 12)[e0:e1]
    first = np.full(n, -1, np.int64)
    first[idx[::-1]] = np.arange(idx.size - 1, -1, -1)      # a triangle's first entry (split references repeat it)
    have = first >= 0
    P = np.zeros((n, 9), np.float32)
    for a in range(0, n, 1 << 20):
        sel = np.nonzero(have[a:a + (1 << 20)])[0] + a
        w = woop[first[sel]].astype(np.float64)
        inv = np.zeros((sel.size, 4, 4))
        inv[:, 0], inv[:, 1] = w[:, 4:8], w[:, 8:12]
        inv[:, 2, :3], inv[:, 2, 3] = w[:, 0:3], -w[:, 3]
        inv[:, 3, 3] = 1.0
        ok = np.abs(np.linalg.det(inv)) > 0
        m = np.zeros_like(inv)
        m[ok] = np.linalg.inv(inv[ok])
        c = m[:, :3, 3]
        P[sel] = np.concatenate([m[:, :3, 0] + c, m[:, :3, 1] + c, c], 1).astype(np.float32)
    P[~np.isfinite(P).all(axis=1)] = 0
    return P, int((~have).sum())


def measure(ctl, torch, dev, desc, mesh, P, a, label):
    pt = ctl.PathTracer(0)
    out = {"mesh": label, "triangles": int(P.shape[0])}
    try:
        t0 = time.perf_counter()
        pt.upload_scene(desc)
        out["upload_s"] = round(time.perf_counter() - t0, 3)
        pt.generate_samples(0)
        n = pt.camera_rays()
        rays = torch.zeros((n, 8), dtype=torch.float32, device=dev)
        hits = torch.zeros((n, 4), dtype=torch.int32, device=dev)
        pt.camera_rays(rays.data_ptr(), n)

        def rate():
            ms = []
            for k in range(a.warmup + a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                pt.intersect_buffers(n, rays.data_ptr(), hits.data_ptr(), False)
                e1.record()
                torch.cuda.synchronize()
                if k >= a.warmup:
                    ms.append(e0.elapsed_time(e1))
            med = statistics.median(ms)
            return {"rays": int(n), "ms_median": round(med, 4), "mrays_s": round(n / med / 1e3, 1),
                    "hits": int((hits[:, 2] >= 0).sum().item())}

        out["intersect_uploaded_sbvh"] = rate()
        out["stack_bound_uploaded"] = pt.stack_bound()
        pos = torch.from_numpy(P).to(dev)
        ms, sync = [], []
        for k in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            pt.rebuild_mesh(mesh, pos.data_ptr(), P.shape[0])
            e1.record()
            torch.cuda.synchronize()
            if k == 0:
                out["first_rebuild_ms"] = round(e0.elapsed_time(e1), 3)   # appends the regions and the scratch
            if k >= a.warmup:
                ms.append(e0.elapsed_time(e1))
                sync.append(pt.last_rebuild_ms())
        med = statistics.median(ms)
        out["rebuild"] = {"calls": a.reps, "ms_median": round(med, 4), "ms_min": round(min(ms), 4),
                          "ms_max": round(max(ms), 4), "mtris_per_s": round(P.shape[0] / med / 1e3, 1),
                          "host_ms_to_first_sync_median": round(statistics.median(s[0] for s in sync), 4),
                          "host_ms_second_sync_median": round(statistics.median(s[1] for s in sync), 4)}
        out["intersect_rebuilt_lbvh"] = rate()
        out["stack_bound_rebuilt"] = pt.stack_bound()
        out["lbvh_over_sbvh_rate"] = round(out["intersect_rebuilt_lbvh"]["mrays_s"] /
                                           out["intersect_uploaded_sbvh"]["mrays_s"], 4)
    finally:
        pt.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=1024, help="grid of n x n quads (0: skip)")
    ap.add_argument("--skip-c3", action="store_true")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import cudatracerlib_amd as ctl
    from cudatracerlib_amd import _abi
    from buildid import source_fingerprint
    dev = torch.device("cuda:0")
    res = {"tool": "tools/mesh_rebuild_bench.py", "device": torch.cuda.get_device_name(0),
           "lib_sha256": hashlib.sha256(open(_abi.LIB_PATH, "rb").read()).hexdigest(),
           "src_sha256": source_fingerprint(ROOT), "warmup": a.warmup, "reps": a.reps,
           "anim_rotation_rebuild_ms_at_grid_size": 0.556, "runs": []}
    threads = max(1, int(os.environ.get("OMP_NUM_THREADS", "8")))
    if a.grid:
        tab = load_module("tools_anim_bench", os.path.join(ROOT, "tools", "tools_anim_bench.py"))
        V, N, BI, BW, T, UV = tab.grid(a.grid, 16)
        T = np.ascontiguousarray(T, np.uint32).reshape(-1, 3)
        s = ctl.HostScene()
        s.add_mesh(V, T, [ctl.diffuse_material(0.5, 0.5, 0.5)])
        s.add_node(0)
        s.set_camera([0, 8, -20], [0, 0, 0], [0, 1, 0], 50, 1024, 1024)
        t0 = time.perf_counter()
        d = s.compile(threads=threads)
        sec = time.perf_counter() - t0
        P = np.ascontiguousarray(V[T].reshape(-1, 9), np.float32)
        r = measure(ctl, torch, dev, d, 0, P, a, f"grid {a.grid}x{a.grid} quads (bench.py's animation leg, static)")
        r["host_compile_s"] = round(sec, 2)
        r["host_compile_threads"] = threads
        res["runs"].append(r)
        s.close()
    if not a.skip_c3:
        bench = load_module("bench", os.path.join(ROOT, "bench.py"))
        ba = bench.parse([])
        t0 = time.perf_counter()
        owner, d, src = bench.kept_scene(ctl, ba, bench.scene_threads())
        sec = time.perf_counter() - t0
        sizes = sorted(d.meshes[i].triangle_offset for i in range(d.n_meshes)) + [d.n_tri_data]
        count = {d.meshes[i].triangle_offset: sizes[sizes.index(d.meshes[i].triangle_offset) + 1] -
                 d.meshes[i].triangle_offset for i in range(d.n_meshes)}
        m = max(range(d.n_meshes), key=lambda i: count[d.meshes[i].triangle_offset])
        P, dropped = positions_from_woop(d, m)
        label = f"mesh {m} of bench.py's default scene (config {ba.config}, {d.n_meshes} meshes, {d.n_nodes} nodes)"
        try:
            r = measure(ctl, torch, dev, d, m, P, a, label)
        except ctl.CTLError as e:     # e.g. a mesh that carries the scene's area light
            r = {"mesh": label, "triangles": int(P.shape[0]), "error": str(e)}
        r["scene_source"] = src
        r["host_compile_s"] = round(sec, 2) if src.startswith("compiled") else None
        r["host_compile_threads"] = bench.scene_threads()
        r["triangles_without_an_entry"] = dropped
        res["runs"].append(r)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
