"""One homogeneous participating medium on the CPU: the host evaluator (ctl_host_medium_eval) against a
float64 statement of the five operations (media_ref.py), edge rays with exact expectations, the record's
layout against the C header, the compiled record and the scene cache."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import media_cases as MC
import media_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = None


@pytest.fixture(scope="module", autouse=True)
def _abi(ctl):
    global A
    A = ctl._abi


# ---------------------------------------------------------------------------------------------
# Tolerances, from the fp32 roundings (EPS = 2^-24 each) and the conditioning of each output.
#
# Volume-space ray.  o = M ori + m and d = M dir are sums of four (three) products.  The library's M is
# the fp32 inverse of the fp32 to_world, the reference's the float64 inverse: for the boxes here (edges 3
# to 5, condition number < 2) that moves an entry by a few EPS of the largest entry.  With S the largest
# sum of |M_ij ori_j| + |m_i| and R the largest row sum of |M_ij| (|dir| = 1):
#     |delta o| <= 12 EPS S,     |delta d| <= 10 EPS R.
# A slab distance t = (b - o) / d on the axis that decides a bound therefore carries
#     |delta t| <= (12 EPS S + |t| 10 EPS R) / |d| + 2 EPS |t|                     (T_TOL below)
# and a bound that tmin or tmax decides is exact.  The hit flag is `t1 > t0 and t1 > 0`: a query is left
# out when t1 - t0 or t1 lies within the two distances' tolerances of zero.
#
# Transmittance exp(-sig_t L), L = |ray(t0) - ray(t1)|: the two points carry 3 EPS (|ori| + |t|) each, so
# |delta L| <= dt0 + dt1 + 6 EPS (|ori| + |t0| + |t1|), and the value's error is T (sig_t |delta L| + EPS
# (3 + 2 sig_t L)): the product's and the exponent's roundings, and cr_exp's own.
#
# Distance sample.  u' = 3 u / w - channel cancels: |delta u'| <= 9 EPS.  sd = -log(1 - u') / sig_t:
# |delta sd| <= (9 EPS / (1 - u') + 3 EPS |log(1 - u')|) / sig_t.  t = tmin + sd adds EPS t, p = ori + t dir
# adds 3 EPS (|ori| + t).  On failure the distance is tmax - tmin, one rounding.  transmittance and the
# two pdfs are sums of exp(-sig_t dist) terms: relative error sig_t |delta dist| + EPS (4 + 2 sig_t dist),
# doubled for the pdfs' averages and the weight's own two roundings.
# Left out (the issue's exclusion rule): |u - w| < 1e-6; 3 u / w within 1e-5 of a channel boundary; the
# sampled distance within its tolerance (plus 1e-6 relative) of tmax - tmin; the largest transmittance
# within 1e-3 relative of 1e-8.  |g| against EPSILON has no margin to apply: g is a constant of each set,
# 0 and 1e-9 on one side and 0.3 and 0.9 on the other.
#
# Phase value (HG).  temp = 1 + g^2 + 2 g cos: |delta temp| <= EPS (3 (1 + |g|)^2 + 2 |g| 4), because the
# dot product of two unit vectors carries 4 EPS; the value is temp^-1.5 times rounded constants:
# relative error 1.5 |delta temp| / temp + 6 EPS.  temp >= (1 - |g|)^2 = 0.01 at |g| = 0.9.
# The point is left out when a volume coordinate lies within 1e-5 of 0 or 1 (|delta o| above is < 2e-6).
#
# Phase sample.  The cosine: 1 - 2 u carries 1 EPS (x2 for the product).  HG's
#     sq = (1 - g^2) / (1 - g + 2 g u),  cos = (1 + g^2 - sq^2) / (2 g)
# has its denominator >= 1 - |g| with error 3 EPS (1 + |g|), so sq <= 1 + |g| carries the relative error
# rs = 3 EPS (1 + |g|) / (1 - |g|) + 3 EPS, and
#     |delta cos| <= (2 (1 + |g|)^2 rs + 3 EPS (1 + g^2 + (1 + |g|)^2)) / (2 |g|) + EPS        (DC below).
# sin = sqrt(1 - cos^2) turns that into a direction error of min(DC / sin, sqrt(2 DC)) + DC; the angle
# 2 pi u (2 EPS relative on up to 2 pi: 8e-7 of sin), the frame (12 EPS) and the three products (6 EPS)
# add 32 EPS.  The frame's branch |x| > |y| of -wi is left out within 1e-6.  The pdf is checked against
# the reference's phase value at the direction the library returned, with the phase value's tolerance.
EPS = 2.0 ** -24
MAX_EXCLUDED = 0.02


def _S_R(V, ori):
    M = np.abs(V["w2v"])
    S = (np.abs(np.asarray(ori, np.float64)) @ M[:3, :3].T + M[:3, 3]).max()
    return S, M[:3, :3].sum(axis=1).max()


def t_tol(V, ori, t, d_axis):
    S, R = _S_R(V, ori)
    t = np.abs(t)
    with np.errstate(invalid="ignore"):
        return np.where(np.isinf(d_axis), 0.0, (12 * EPS * S + t * 10 * EPS * R) / d_axis) + 2 * EPS * t


def sampled_distance_tol(ref):
    with np.errstate(divide="ignore", invalid="ignore"):
        dsd = np.where(ref["tried"], (9 * EPS / (1 - ref["u1"]) + 3 * EPS * np.abs(np.log1p(-ref["u1"]))) /
                       ref["sig_t"][ref["channel"]], 0.0)
    return np.where(np.isfinite(dsd), dsd, 0.0)     # a channel without extinction: the distance is infinite


def kept(V, op, q, ref):
    """The exclusion rule: the queries of a set that stay in, from the float64 reference and the inputs alone
    (no library result enters).  Every margin of the header comment is here and nowhere else."""
    if op in ("intersect", "transmittance", "phase_sample"):
        box = ref["meets_box"] if op == "phase_sample" else ref
        dt0, dt1 = t_tol(V, q["ori"], box["t0"], box["d_lo"]), t_tol(V, q["ori"], box["t1"], box["d_hi"])
        keep = (np.abs(box["t1"] - box["t0"]) > dt0 + dt1 + 1e-6) & (np.abs(box["t1"]) > dt1 + 1e-6)
        if op == "phase_sample":
            keep &= ref["xy_gap"] > 1e-6
        return keep
    if op == "sample_distance":
        dsd = sampled_distance_tol(ref)
        keep = np.abs(q["u"][:, 0].astype(np.float64) - ref["weight"]) > 1e-6
        frac = ref["v"] - np.floor(ref["v"])
        keep &= ~ref["tried"] | ((frac > 1e-5) & (frac < 1 - 1e-5)) | (ref["v"] < 0.5)
        keep &= ~ref["tried"] | ~np.isfinite(ref["sd"]) | (np.abs(ref["sd"] - ref["span"]) > dsd + 1e-6 * ref["span"])
        keep &= np.abs(ref["tr_max"] / 1e-8 - 1) > 1e-3
        return keep
    assert op == "phase_eval"
    pl = ref["pl"]
    return np.all((np.abs(pl) > 1e-5) & (np.abs(pl - 1) > 1e-5), axis=1)


def check_intersect(V, q, got, ref, with_transmittance=False):
    n = q.shape[0]
    dt0, dt1 = t_tol(V, q["ori"], ref["t0"], ref["d_lo"]), t_tol(V, q["ori"], ref["t1"], ref["d_hi"])
    keep = kept(V, "intersect", q, ref)
    hit = keep & ref["hit"]
    assert np.array_equal(got["hit"][keep] != 0, ref["hit"][keep])
    miss = keep & ~ref["hit"]
    assert not got["t0"][miss].any() and not got["t1"][miss].any()
    e0, e1 = np.abs(got["t0"][hit] - ref["t0"][hit]), np.abs(got["t1"][hit] - ref["t1"][hit])
    assert np.all(e0 <= dt0[hit]) and np.all(e1 <= dt1[hit]), (float((e0 - dt0[hit]).max()), float((e1 - dt1[hit]).max()))
    worst = max((e0 / np.maximum(dt0[hit], 1e-300)).max(initial=0), (e1 / np.maximum(dt1[hit], 1e-300)).max(initial=0))
    if with_transmittance:
        sig_t = (V["sig_a"].astype(np.float64) + V["sig_s"])[None, :]
        o = np.linalg.norm(q["ori"].astype(np.float64), axis=1)
        dL = np.where(ref["hit"], dt0 + dt1 + 6 * EPS * (o + np.abs(ref["t0"]) + np.abs(ref["t1"])), 0.0)
        T = ref["transmittance"]
        tol = T * (sig_t * dL[:, None] + EPS * (3 + 2 * sig_t * ref["length"][:, None]))
        err = np.abs(got["transmittance"] - T)
        assert np.all(err[keep] <= tol[keep]), float((err[keep] / np.maximum(tol[keep], 1e-300)).max())
        assert np.all(got["transmittance"][miss] == 1.0)
        worst = max(worst, (err[keep] / np.maximum(tol[keep], 1e-300)).max())
    assert hit.sum() > n // 8 and miss.sum() > n // 8
    return keep, worst


def check_sample_distance(V, q, got, ref):
    n = q.shape[0]
    w, sig_t = ref["weight"], ref["sig_t"]
    dsd = sampled_distance_tol(ref)
    keep = kept(V, "sample_distance", q, ref)
    ins, out = keep & ref["inside"], keep & ~ref["inside"]
    assert np.array_equal(got["hit"][keep] != 0, ref["success"][keep])
    # outside: the distance is tmax - tmin (one rounding of it); t, p and the coefficients stay unwritten
    for f in ("t", "p", "sigma_a", "sigma_s"):
        assert not got[f][out].any(), f
    assert np.array_equal(got["sigma_a"][ins], np.broadcast_to(V["sig_a"], got["sigma_a"][ins].shape))
    assert np.array_equal(got["sigma_s"][ins], np.broadcast_to(V["sig_s"], got["sigma_s"][ins].shape))
    ddist = np.where(ref["inside"], dsd, EPS * np.minimum(ref["span"], 1e30))
    o = np.linalg.norm(q["ori"].astype(np.float64), axis=1)
    dt = ddist + EPS * np.abs(ref["t"])
    worst = {}
    e = np.abs(got["t"][ins] - ref["t"][ins])
    assert np.all(e <= dt[ins]), float((e / dt[ins]).max())
    worst["t"] = (e / np.maximum(dt[ins], 1e-300)).max(initial=0)
    dp = dt + 3 * EPS * (o + np.abs(ref["t"]))
    e = np.linalg.norm(got["p"][ins] - ref["p"][ins], axis=1)
    assert np.all(e <= dp[ins]), float((e / dp[ins]).max())
    worst["p"] = (e / dp[ins]).max(initial=0)
    finite = keep & (ref["dist"] < 1e30)
    rel = sig_t[None, :] * ddist[:, None] + EPS * (4 + 2 * sig_t[None, :] * np.minimum(ref["dist"], 1e30)[:, None])
    tolT = ref["transmittance"] * rel
    e = np.abs(got["transmittance"] - ref["transmittance"])
    assert np.all(e[finite] <= tolT[finite]), float((e[finite] / np.maximum(tolT[finite], 1e-300)).max())
    worst["transmittance"] = (e[finite] / np.maximum(tolT[finite], 1e-300)).max(initial=0)
    relmax = 2 * rel.max(axis=1) + 4 * EPS
    for f in ("pdf_success", "pdf_failure"):
        e = np.abs(got[f] - ref[f])
        tol = relmax * np.maximum(np.abs(ref[f]), abs(w) * np.mean(sig_t) if f == "pdf_success" else 1.0)
        assert np.all(e[finite] <= tol[finite]), (f, float((e[finite] / np.maximum(tol[finite], 1e-300)).max()))
        worst[f] = (e[finite] / np.maximum(tol[finite], 1e-300)).max(initial=0)
    assert np.array_equal(got["pdf_success"].view(np.uint32), got["pdf_success_rev"].view(np.uint32))
    # tmax = FLT_MAX and no sample inside: the medium is opaque over an unbounded distance
    far = keep & ~ref["inside"] & (ref["dist"] >= 1e30)
    lit = sig_t > 0
    assert not got["transmittance"][far][:, lit].any()
    return keep, worst


def check_phase_eval(V, q, got, ref):
    keep = kept(V, "phase_eval", q, ref)
    g = abs(V["g"]) if V["phase"] == "hg" else 0.0
    dtemp = EPS * (3 * (1 + g) ** 2 + 8 * g)
    tol = ref["value"] * (1.5 * dtemp / ref["temp"] + 6 * EPS)
    e = np.abs(got["value"] - ref["value"])
    assert np.all(e[keep] <= tol[keep]), float((e[keep] / np.maximum(tol[keep], 1e-300)).max())
    outside = keep & ~ref["inside"]
    assert not got["value"][outside].any()
    if np.mean(V["sig_s"]) != 0:
        assert outside.sum() > q.shape[0] // 4 and (keep & ref["inside"]).sum() > q.shape[0] // 8
    else:
        assert not got["value"].any()
    return keep, (e[keep] / np.maximum(tol[keep], 1e-300)).max(initial=0)


def cos_tol(V):
    g = abs(V["g"]) if V["phase"] == "hg" else 0.0
    if g < MR.EPSILON:
        return 2 * EPS
    rs = 3 * EPS * (1 + g) / (1 - g) + 3 * EPS
    return (2 * (1 + g) ** 2 * rs + 3 * EPS * (1 + g * g + (1 + g) ** 2)) / (2 * g) + EPS


def check_phase_sample(V, q, got, ref):
    n = q.shape[0]
    mb = ref["meets_box"]
    keep = kept(V, "phase_sample", q, ref)
    assert np.array_equal(got["hit"][keep] != 0, mb["hit"][keep])
    miss, hit = keep & ~mb["hit"], keep & mb["hit"]
    for f in ("wo_out", "value", "pdf"):
        assert not got[f][miss].any()
    assert np.all(got["value"][hit] == 1.0)
    dc = cos_tol(V)
    tol = np.minimum(dc / np.maximum(ref["sin_theta"], 1e-300), np.sqrt(2 * dc)) + dc + 32 * EPS
    e = np.linalg.norm(got["wo_out"] - ref["wo"], axis=1)
    assert np.all(e[hit] <= tol[hit]), float((e[hit] / tol[hit]).max())
    val, temp = MR.phase_value(V, q["dir"], got["wo_out"])
    g = abs(V["g"]) if V["phase"] == "hg" else 0.0
    ptol = val * (1.5 * EPS * (3 * (1 + g) ** 2 + 8 * g) / temp + 6 * EPS)
    pe = np.abs(got["pdf"] - val)
    assert np.all(pe[hit] <= ptol[hit]), float((pe[hit] / ptol[hit]).max())
    assert hit.sum() > n // 4
    return keep, max((e[hit] / tol[hit]).max(), (pe[hit] / ptol[hit]).max())


def check_set(name, op, q, got, ref):
    V = MC.VOLUMES[name]
    if op == "intersect":
        keep, worst = check_intersect(V, q, got, ref)
    elif op == "transmittance":
        keep, worst = check_intersect(V, q, got, ref, with_transmittance=True)
    elif op == "sample_distance":
        keep, worst = check_sample_distance(V, q, got, ref)
    elif op == "phase_eval":
        keep, worst = check_phase_eval(V, q, got, ref)
    else:
        keep, worst = check_phase_sample(V, q, got, ref)
    left_out = int((~keep).sum())
    print(f"{name} {op}: worst error / tolerance {worst}, left out {left_out} of {q.shape[0]}")
    assert left_out <= MAX_EXCLUDED * q.shape[0], (name, op, left_out)


def test_host_evaluator_against_float64(ctl):
    sets = MC.random_sets(ctl)
    assert {op for _, op, _, _ in sets} == set(MC.OPS)
    assert all(q.shape[0] == 4096 for name, _, q, _ in sets if name == "tilted_hg")
    for name, op, q, ref in sets:
        _, d = MC.eval_scene(ctl, name)
        check_set(name, op, q, ctl.host_medium_eval(d, q), ref)


def test_reference_alone_stays_inside_the_cap(ctl):
    """Every margin of the exclusion rule (kept: the slab distances against their tolerances, u against the
    sampling weight, the channel boundaries, the sampled distance against the interval, the 1e-8 flush, the
    box faces, the frame's branch), applied to every random set from the float64 reference and the inputs
    alone: no library result is looked at, and no set loses more than the cap.  With margins of order 1e-6 to
    1e-5 on uniform draws the expected share is of order 1e-5 to 1e-4; a fifth of the cap is asserted."""
    worst = 0.0
    for name, op, q, ref in MC.random_sets(ctl):
        keep = kept(MC.VOLUMES[name], op, q, ref)
        share = (~keep).sum() / q.shape[0]
        worst = max(worst, share)
        assert share <= MAX_EXCLUDED / 5, (name, op, int((~keep).sum()))
    print(f"largest share left out by the margins alone: {worst:.5f}")


def test_edge_rays_on_the_host(ctl):
    _, d = MC.eval_scene(ctl, "axis_iso")
    sig_t = np.float64(1.0)
    for op in ("intersect", "transmittance"):
        for name, (q, hit, t0, t1) in MC.edge_rays(ctl, op).items():
            r = ctl.host_medium_eval(d, q)
            assert (int(r["hit"][0]), float(r["t0"][0]), float(r["t1"][0])) == (hit, t0, t1), (op, name)
            if op == "transmittance":
                want = np.float32(np.exp(-sig_t * np.float64(np.float32(t1 - t0)))) if hit else np.float32(1)
                assert np.all(r["transmittance"][0] == want), name
    # a ray in a face's plane and parallel to it (0 / 0 in the slab test) is answered, and twice the same
    q = MC.queries(ctl, "intersect", [(2.0, 0.0, -4.0)], [(0.0, 0.0, 1.0)])
    a, b = ctl.host_medium_eval(d, q), ctl.host_medium_eval(d, q)
    assert a.tobytes() == b.tobytes() and np.isfinite(a["t0"]).all()


def test_edge_samples_on_the_host(ctl):
    # sig_s = 0: every albedo is 0, so is the sampling weight, no distance is ever sampled, and going
    # through weighs transmittance / pdf_failure with pdf_failure = 0 * avg + 1
    _, d = MC.eval_scene(ctl, "absorbing")
    q = MC.queries(ctl, "sample_distance", [(0, 0, 0)] * 4, [(0, 0, 1)] * 4, 0.0, 1.5, u=[(0, 0), (0.25, 0), (0.5, 0), (0.999, 0)])
    r = ctl.host_medium_eval(d, q)
    assert not r["hit"].any() and not r["t"].any() and not r["pdf_success"].any() and np.all(r["pdf_failure"] == 1)
    T = np.exp(-np.float64(1.5) * MC.VOLUMES["absorbing"]["sig_a"].astype(np.float64))
    assert np.abs(r["transmittance"] - T).max() < 4e-7
    # sig_t = 0 on the red channel: a draw that picks it samples an infinite distance and fails
    _, d = MC.eval_scene(ctl, "empty_channel")
    w = MR.sampling_weight(MC.VOLUMES["empty_channel"])
    assert w == 0.75
    q = MC.queries(ctl, "sample_distance", [(0, 0, 0)] * 2, [(0, 0, 1)] * 2, 0.0, 1.0, u=[(0.125, 0), (0.375, 0)])
    r = ctl.host_medium_eval(d, q)
    assert r["hit"][0] == 0 and r["transmittance"][0, 0] == 1.0 and r["hit"][1] == 1
    # p == ray origin: a sampled distance of 0 (u = 0) does not count as an interaction
    _, d = MC.eval_scene(ctl, "axis_iso")
    r = ctl.host_medium_eval(d, MC.queries(ctl, "sample_distance", [(0, 0, 0)], [(0, 0, 1)], 0.0, 1.0, u=(0.0, 0.0)))
    assert r["hit"][0] == 0 and r["t"][0] == 0 and np.all(r["transmittance"][0] == 1)
    # a transmittance below 1e-8 on every channel leaves as 0
    r = ctl.host_medium_eval(d, MC.queries(ctl, "sample_distance", [(0, 0, 0)], [(0, 0, 1)], 0.0, 19.0, u=(0.9999, 0.0)))
    assert r["hit"][0] == 0 and not r["transmittance"].any() and r["pdf_failure"][0] > 0
    # tmax = FLT_MAX with a sample inside
    r = ctl.host_medium_eval(d, MC.queries(ctl, "sample_distance", [(0, 0, 0)], [(0, 0, 1)], 0.0, MC.FLT_MAX, u=(0.3125, 0.0)))
    assert r["hit"][0] == 1 and np.isfinite(r["t"][0]) and r["t"][0] > 0
    # a scene without a volume, and an op outside the five: all zero
    _, d0 = MC.eval_scene(ctl, None)
    q = MC.queries(ctl, "transmittance", [(0, 0, -3)], [(0, 0, 1)])
    assert not ctl.host_medium_eval(d0, q).view(np.uint8).any()
    q["op"] = 77
    assert not ctl.host_medium_eval(d, q).view(np.uint8).any()


# ---------------------------------------------------------------------------------------------
def test_layouts_match_header(ctl, tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    structs = [("ctl_volume", "Volume"), ("ctl_medium_query", "MediumQuery"), ("ctl_medium_result", "MediumResult"),
               ("ctl_scene_desc", "SceneDesc")]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ctl_trace.h"', 'int main(void) {']
    expect = []
    for cname, pname in structs:
        py = getattr(A, pname)
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        expect.append(C.sizeof(py))
        for fld in py._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {fld[0]}));')
            expect.append(getattr(py, fld[0]).offset)
    for name in ("CTL_DIRTY_VOLUMES", "CTL_DIRTY_ALL", "CTL_MAX_NUM_VOLUMES", "CTL_VOLUME_HOMOGENEOUS", "CTL_PHASE_ISOTROPIC",
                 "CTL_PHASE_HG", "CTL_MEDIUM_INTERSECT", "CTL_MEDIUM_TRANSMITTANCE", "CTL_MEDIUM_SAMPLE_DISTANCE",
                 "CTL_MEDIUM_PHASE_EVAL", "CTL_MEDIUM_PHASE_SAMPLE"):
        lines.append(f'printf("%zu\\n", (size_t){name});')
        expect.append(getattr(A, name))
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == expect
    assert C.sizeof(A.Volume) == 176 and C.sizeof(A.Volume) % 16 == 0
    assert A.CTL_DIRTY_VOLUMES == 1 << 10 and A.CTL_DIRTY_ALL == (1 << 11) - 1
    assert ctl.MEDIUM_QUERY_DTYPE.itemsize == C.sizeof(A.MediumQuery) == 56
    assert ctl.MEDIUM_RESULT_DTYPE.itemsize == C.sizeof(A.MediumResult) == 96
    for dt, st in ((ctl.MEDIUM_QUERY_DTYPE, A.MediumQuery), (ctl.MEDIUM_RESULT_DTYPE, A.MediumResult)):
        assert [(n, dt.fields[n][1]) for n in dt.names] == [(f[0], getattr(st, f[0]).offset) for f in st._fields_]


def test_compiled_record(ctl):
    for name in ("tilted_hg", "axis_iso"):
        V = MC.VOLUMES[name]
        _, d = MC.eval_scene(ctl, name)
        assert d.n_volumes == 1
        r = d.volumes[0]
        assert (r.kind, r.phase) == (A.CTL_VOLUME_HOMOGENEOUS, A.CTL_PHASE_HG if V["phase"] == "hg" else A.CTL_PHASE_ISOTROPIC)
        assert r.phase_g == np.float32(V["g"]) and not any(r.le[:])
        assert np.array_equal(np.array(r.sig_a[:], np.float32), V["sig_a"]) and np.array_equal(np.array(r.sig_s[:], np.float32), V["sig_s"])
        v2w = np.array(r.volume_to_world.m[:], np.float32).reshape(4, 4)
        w2v = np.array(r.world_to_volume.m[:], np.float64).reshape(4, 4)
        assert np.array_equal(v2w, V["to_world"])
        # the fp32 inverse of a matrix with entries up to 5 and condition number < 2: a few 2^-24 of 5
        assert np.abs(w2v @ v2w.astype(np.float64) - np.eye(4)).max() < 2e-6
    _, d0 = MC.eval_scene(ctl, None)
    assert d0.n_volumes == 0 and not d0.volumes


def test_compiler_refusals(ctl):
    inf, nan = float("inf"), float("nan")
    s = ctl.HostScene()
    ok = dict(to_world=MC.AXIS_BOX, sigma_a=(0.25, 0.25, 0.25), sigma_s=(0.5, 0.5, 0.5))
    bad_m = MC.AXIS_BOX.copy()
    bad_m[1, 3] = nan
    singular = MC.AXIS_BOX.copy()
    singular[:3, :3] = 0
    for over, match in ((dict(sigma_a=(0.25, nan, 0.25)), "non-finite"), (dict(sigma_s=(inf, 0.5, 0.5)), "non-finite"),
                        (dict(le=(0, nan, 0)), "non-finite"), (dict(to_world=bad_m), "non-finite"),
                        (dict(to_world=singular), "non-finite"), (dict(sigma_a=(0.25, -0.125, 0.25)), "negative"),
                        (dict(sigma_s=(-1.0, 0.5, 0.5)), "negative"), (dict(phase="hg", g=1.0), "below 1"),
                        (dict(phase="hg", g=-1.5), "below 1"), (dict(phase="hg", g=nan), "non-finite")):
        with pytest.raises(ctl.CTLError, match=match):
            s.add_homogeneous_volume(**{**ok, **over})
    with pytest.raises(ValueError):
        s.add_homogeneous_volume(**{**ok, "phase": "rayleigh"})
    f3 = C.c_float * 3
    m = (C.c_float * 16)(*MC.AXIS_BOX.reshape(16))
    assert s._L.ctl_host_scene_add_homogeneous_volume(s._h, m, f3(1, 1, 1), f3(1, 1, 1), f3(0, 0, 0), 7, 0.0) == -1
    assert s.add_homogeneous_volume(**ok) == 0
    with pytest.raises(ctl.CTLError, match="one volume"):
        s.add_homogeneous_volume(**ok)


def test_host_evaluator_refuses_a_damaged_description(ctl):
    _, d = MC.eval_scene(ctl, "axis_iso")
    q = MC.queries(ctl, "intersect", [(0, 0, -3)], [(0, 0, 1)])
    r = d.volumes[0]
    for field, value, match in (("kind", 9, "kind"), ("phase", 5, "phase"), ("phase_g", 1.0, "below 1")):
        keep = getattr(r, field)
        try:
            setattr(r, field, value)
            with pytest.raises(ctl.CTLError, match=match):
                ctl.host_medium_eval(d, q)
        finally:
            setattr(r, field, keep)
    try:
        d.n_volumes = 2
        with pytest.raises(ctl.CTLError, match="more than one"):
            ctl.host_medium_eval(d, q)
    finally:
        d.n_volumes = 1
    assert ctl.host_medium_eval(d, q)["hit"][0] == 1


def test_scene_cache_round_trip(ctl, tmp_path):
    from cudatracerlib_amd import scene_cache
    _, d = MC.eval_scene(ctl, "tilted_hg")
    path = str(tmp_path / "scene.bin")
    scene_cache.save(d, path)
    c = scene_cache.load(path)
    try:
        assert c.desc.n_volumes == 1
        assert bytes(c.desc.volumes[0]) == bytes(d.volumes[0])
        q = MC.op_set(ctl, "tilted_hg", "sample_distance", 64)[0]
        assert ctl.host_medium_eval(c.desc, q).tobytes() == ctl.host_medium_eval(d, q).tobytes()
    finally:
        c.close()
    # a scene without a volume round-trips to a null pointer
    _, d0 = MC.eval_scene(ctl, None)
    scene_cache.save(d0, path)
    c = scene_cache.load(path)
    try:
        assert c.desc.n_volumes == 0 and not c.desc.volumes
    finally:
        c.close()
    # a file written for the description before the volume members (16 bytes shorter) is refused
    with open(path, "rb") as f:
        head = f.read(16)
        hlen = int.from_bytes(head[8:16], "little")
        h = json.loads(f.read(hlen).decode())
        rest = f.read()
    assert h["desc_size"] == C.sizeof(A.SceneDesc)
    h["desc_size"] -= 16
    at = 2 * A.SceneDesc.volumes.offset              # the two members' 16 bytes, in front of materials_ext
    h["desc"] = h["desc"][:at] + h["desc"][at + 32:]
    del h["arrays"]["volumes"]
    header = json.dumps(h).encode()
    old = str(tmp_path / "old.bin")
    with open(old, "wb") as f:
        f.write(head[:8] + len(header).to_bytes(8, "little") + header + rest)
    with pytest.raises(ValueError, match="another SceneDesc layout"):
        scene_cache.load(old)
