"""dielectric, thindielectric, conductor, roughconductor and plastic on the CPU: ctl_host_bsdf_eval
(the bsdf_sample / bsdf_f / bsdf_pdf dispatch the integrators call) against tests/bsdf_ref.py, the
ABI of the new records, the host compile's ext array, the .xmsh writer and the scene cache.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import bsdf_cases as BC
import bsdf_ref as R
import cudatracerlib_amd as ctl
from cudatracerlib_amd import _abi, scene_cache

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24   # one fp32 rounding, relative


def _eval(q):
    return ctl.host_bsdf_eval(BC.host_scene()[1], q)


def _report(q, got, want, bad):
    i = int(bad[0])
    return (f"{len(bad)} of {len(q)} queries differ; first: query {q[i]} got {got[i]} want {want[i]}")


@pytest.mark.parametrize("type", [R.DIELECTRIC, R.THINDIELECTRIC, R.CONDUCTOR])
def test_delta_types_match_the_restatement_bit_for_bit(type):
    q = BC.delta_queries(type)
    assert len(q) >= 4000
    got, want = _eval(q), BC.reference(q)
    bad = BC.same_bits(got, want)
    assert bad.size == 0, _report(q, got, want, bad)


def _plastic_reference(q):
    """The restatement with the warp taken from the entry's diffuse material (index 0) at the remapped sample."""
    return BC.plastic_reference(q, _eval)


def test_plastic_matches_the_restatement_bit_for_bit():
    q = BC.delta_queries(R.PLASTIC)
    assert len(q) >= 4000
    got = _eval(q)
    want, n_warps = _plastic_reference(q)
    # the diffuse lobe is exercised, with remapped and with plain samples
    assert n_warps >= 50 and (want["sampled_type"] == R.EDIFFUSE_REFLECTION).sum() >= 300
    bad = BC.same_bits(got, want)
    assert bad.size == 0, _report(q, got, want, bad)


def test_delta_queries_reach_every_branch():
    """The directed set is not vacuous: per type, both lobes are sampled, f and pdf accept the exact
    directions under the discrete measure and refuse the ones just past DeltaEpsilon, and total
    internal reflection occurs."""
    for type in (R.DIELECTRIC, R.THINDIELECTRIC, R.CONDUCTOR, R.PLASTIC):
        q = BC.delta_queries(type)
        want = _plastic_reference(q)[0] if type == R.PLASTIC else BC.reference(q)
        s = want[q["op"] == 0]
        lobes = set(int(x) for x in np.unique(s["sampled_type"]))
        assert set(BC.LOBES[type]) & lobes == (set(BC.LOBES[type]) if type != R.CONDUCTOR else {R.EDELTA_REFLECTION}), lobes
        fq = want[(q["op"] == 1) & (q["measure"] == R.EDISCRETE)]
        assert (fq["value"].max(axis=1) > 0).sum() >= 50 and (fq["value"].max(axis=1) == 0).sum() >= 50
        assert (want[(q["op"] == 1) & (q["measure"] == R.ESOLID_ANGLE) & (q["type_mask"] != R.EALL)
                     & (q["type_mask"] != R.EDIFFUSE_REFLECTION) & (q["type_mask"] != 0x22)]["value"] == 0).all()
    q = BC.delta_queries(R.DIELECTRIC)
    want = BC.reference(q)
    tir = (q["op"] == 0) & (q["type_mask"] == (R.EDELTA_REFLECTION | R.EDELTA_TRANSMISSION)) & (want["pdf"] == 1.0)
    assert tir.sum() >= 20


# ---------------------------------------------------------------------------------------------
# roughconductor: its microfacet steps (mf_eval, mf_G, mf_smithG1, mf_sample) are the rough
# dielectric's, held to a float64 reference from the papers in tests/test_microfacet_host.py (as is
# the rough conductor itself); what is new is how they are combined.

def _rough_dirs():
    """(wi, wo) with wi.z in [0.6, 0.95] and wo the mirror image of wi about a half vector tilted by
    tan(theta_h) <= 0.25 (the smaller alpha), so D(H) >= D(0) / e^1 or D(0) / 4 and nothing underflows.
    In dot(w, H) the z term is at least 0.6 * 0.97 = 0.58 and the other two at most sin(theta_h)
    sin(theta_w) = 0.243 * 0.8 = 0.19 together, so the sum of the terms' magnitudes is at most
    (0.58 + 0.19) / (0.58 - 0.19) < 2 times the dot product: a dot's 5 roundings count as 10."""
    rng = np.random.RandomState(7)
    out = []
    for _ in range(400):
        cz, phi = rng.uniform(0.6, 0.95), rng.uniform(0, 2 * np.pi)
        wi = np.array([np.sqrt(1 - cz * cz) * np.cos(phi), np.sqrt(1 - cz * cz) * np.sin(phi), cz])
        t, ph = rng.uniform(0.0, 0.25), rng.uniform(0, 2 * np.pi)
        h = np.array([t * np.cos(ph), t * np.sin(ph), 1.0])
        h /= np.linalg.norm(h)
        wo = 2 * np.dot(wi, h) * h - wi
        assert wo[2] > 0.05
        out.append((wi.astype(np.float32), wo.astype(np.float32)))
    return out


def _rough_pairs():
    _, D = BC.materials()
    rc, rd = BC.indices_of(R.ROUGHCONDUCTOR), BC.indices_of(5)
    return [(c, d) for c in rc for d in rd if D[c]["dist"] == D[d]["dist"]]


def test_roughconductor_f_and_pdf_against_the_rough_dielectric():
    """f_rc / F_conductor == f_rd(reflection lobe) / F_dielectric and pdf_rc == pdf_rd(reflection only).

    Roundings (each at most 2^-24 relative; both chains share H = normalize(wo + wi), D, G, G1):
      f:   rc  D*G, / (4 wi.z), F*value                    3      (4 wi.z and R = 1 are exact)
           rd  F*D, *G, / (4 |wi.z|)                       3   -> bound 6 * 2^-24
      pdf: rc  D*G1, / (4 wi.z)                            2
           rd  dot(wi,H) 10, G1*absdot 1, *D 1, / |wi.z| 1, dot(wo,H) 10, 1/(4 dot) 1, prob*dwh 1   25
               (a dot's 5 roundings count twice for these directions, see _rough_dirs)
           and dot(wi,H) = dot(wo,H) holds up to the unit-length defect of the two fp32 input vectors
           (three rounded components each, 2^-24 relative per squared component, over a dot product
           of at least 0.39: 6 / 0.39)                                                         16
                                                                                      -> bound 43 * 2^-24
    F_conductor and F_dielectric at dot(wi, H) come from the restatement (+ - * / sqrt only)."""
    dirs = _rough_dirs()
    pairs = _rough_pairs()
    assert len(pairs) == 2
    _, D = BC.materials()
    worst_f = worst_p = 0.0
    skipped = total = 0
    for c, d in pairs:
        q = np.zeros(4 * len(dirs), dtype=ctl.BSDF_QUERY_DTYPE)
        for i, (wi, wo) in enumerate(dirs):
            q[4 * i + 0] = (c, 1, R.EALL, R.ESOLID_ANGLE, wi, wo, (0, 0), (0, 0))
            q[4 * i + 1] = (d, 1, R.EGLOSSY_REFLECTION, R.ESOLID_ANGLE, wi, wo, (0, 0), (0, 0))
            q[4 * i + 2] = (c, 2, R.EALL, R.ESOLID_ANGLE, wi, wo, (0, 0), (0, 0))
            q[4 * i + 3] = (d, 2, R.EGLOSSY_REFLECTION, R.ESOLID_ANGLE, wi, wo, (0, 0), (0, 0))
        res = _eval(q)
        for i, (wi, wo) in enumerate(dirs):
            total += 1
            wi_, wo_ = R.vec(wi), R.vec(wo)
            H = R.normalize((wo_[0] + wi_[0], wo_[1] + wi_[1], wo_[2] + wi_[2]))
            Fc = np.array(R.fresnel_conductor_exact(R.dot(wi_, H), BC.GOLD_ETA, BC.GOLD_K), np.float64)
            Fd = float(R.fresnel_dielectric_ext(R.dot(wi_, H), np.float32(1.5))[0])
            f_rc, f_rd = res[4 * i]["value"].astype(np.float64), float(res[4 * i + 1]["value"][0])
            p_rc, p_rd = float(res[4 * i + 2]["pdf"]), float(res[4 * i + 3]["pdf"])
            if f_rd == 0.0 or Fd == 0.0 or p_rd == 0.0:
                skipped += 1
                continue
            want = Fc * (f_rd / Fd)
            worst_f = max(worst_f, float(np.abs(f_rc / want - 1.0).max()))
            worst_p = max(worst_p, abs(p_rc / p_rd - 1.0))
    print(f"roughconductor: f worst {worst_f / U:.2f} roundings, pdf worst {worst_p / U:.2f} roundings, "
          f"{skipped} of {total} skipped")
    assert skipped <= 0.05 * total
    assert worst_f <= 6 * U * (1 + 1e-3)
    assert worst_p <= 43 * U * (1 + 1e-3)
    # the discrete measure and the wrong hemisphere give nothing
    wi, wo = dirs[0]
    q = np.zeros(3, dtype=ctl.BSDF_QUERY_DTYPE)
    c = pairs[0][0]
    q[0] = (c, 1, R.EALL, R.EDISCRETE, wi, wo, (0, 0), (0, 0))
    q[1] = (c, 2, R.EALL, R.ESOLID_ANGLE, wi, -wo, (0, 0), (0, 0))
    q[2] = (c, 1, R.EALL & ~R.EGLOSSY_REFLECTION, R.ESOLID_ANGLE, wi, wo, (0, 0), (0, 0))
    res = _eval(q)
    assert not res["value"].any() and not res["pdf"].any()


def test_roughconductor_sample_weight_is_f_over_pdf():
    """sample's weight F(wi.m) G1(wo, m) against f / pdf of the entry at the sampled wo (the reference's
    f carries the cosine factor, so f / pdf is the whole weight), and its pdf against pdf.

    f / pdf = F(wi.H) G1(wo, H) with H = normalize(wo + wi) where the sample used m, and wo =
    reflect(wi, m).  Roundings: f 4 (G1*G1, D*G, /, F*value), pdf 2, the weight's product 1; H differs
    from m by the roundings of reflect (dot 5, 2*dot, *n, -wi, normalize 8: 16) and of H itself
    (add, normalize 8: 9), 25 in all, which F and G1 pass on with a condition number below 2 for the
    cosines >= 0.3 used here: bound (7 + 2 * 25) * 2^-24 = 57 * 2^-24.  The pdf chains: sample 2 more
    than pdf's (its |wi.m| / (4 wo.m) in place of 1 / 4), D and G1 at m against H through the same 25
    roundings with a condition number below 1 / alpha^2 < 16: bound (6 + 16 * 25) * 2^-24."""
    rng = np.random.RandomState(11)
    _, D = BC.materials()
    worst_w = worst_p = 0.0
    skipped = total = 0
    for c in BC.indices_of(R.ROUGHCONDUCTOR):
        n = 300
        q = np.zeros(n, dtype=ctl.BSDF_QUERY_DTYPE)
        for i in range(n):
            cz, phi = rng.uniform(0.9, 0.99), rng.uniform(0, 2 * np.pi)   # near-normal wi: few grazing wo
            a = np.array([np.sqrt(1 - cz * cz) * np.cos(phi), np.sqrt(1 - cz * cz) * np.sin(phi), cz])
            smp = (rng.uniform(0.05, 0.6), rng.uniform(0.05, 0.95))        # sample.x off the distribution's tail
            q[i] = (c, 0, R.EALL, R.ESOLID_ANGLE, a.astype(np.float32), (0, 0, 1), smp, (0, 0))
        s = _eval(q)
        q2 = np.zeros(2 * n, dtype=ctl.BSDF_QUERY_DTYPE)
        for i in range(n):
            q2[2 * i] = (c, 1, R.EALL, R.ESOLID_ANGLE, q[i]["wi"], s[i]["wo"], (0, 0), (0, 0))
            q2[2 * i + 1] = (c, 2, R.EALL, R.ESOLID_ANGLE, q[i]["wi"], s[i]["wo"], (0, 0), (0, 0))
        r = _eval(q2)
        for i in range(n):
            total += 1
            f, p = r[2 * i]["value"].astype(np.float64), float(r[2 * i + 1]["pdf"])
            if float(s[i]["pdf"]) == 0.0 or p == 0.0 or not s[i]["value"].all() or s[i]["wo"][2] < 0.3:
                skipped += 1   # rejected samples (pdf 0, wo below the surface) and grazing wo
                continue
            assert int(s[i]["sampled_type"]) == R.EGLOSSY_REFLECTION
            worst_w = max(worst_w, float(np.abs(s[i]["value"].astype(np.float64) / (f / p) - 1.0).max()))
            worst_p = max(worst_p, abs(float(s[i]["pdf"]) / p - 1.0))
    print(f"roughconductor sample: weight worst {worst_w / U:.2f} roundings, pdf worst {worst_p / U:.2f} roundings, "
          f"{skipped} of {total} skipped")
    assert skipped <= 0.05 * total
    assert worst_w <= 57 * U
    assert worst_p <= (6 + 16 * 25) * U


# ---------------------------------------------------------------------------------------------
def test_abi_sizes_and_layouts(tmp_path):
    assert C.sizeof(_abi.Material) == 80
    assert C.sizeof(_abi.MaterialExt) == 64
    assert C.sizeof(_abi.BsdfQuery) == 56 == ctl.BSDF_QUERY_DTYPE.itemsize
    assert C.sizeof(_abi.BsdfResult) == 32 == ctl.BSDF_RESULT_DTYPE.itemsize
    assert _abi.CTL_XMSH_MATERIAL_RECORD_SIZE == 148 and _abi.ABI_VERSION == 4
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    structs = [("ctl_material_ext", _abi.MaterialExt), ("ctl_bsdf_query", _abi.BsdfQuery),
               ("ctl_bsdf_result", _abi.BsdfResult), ("ctl_scene_desc", _abi.SceneDesc)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ctl_trace.h"', 'int main(void) {']
    expect = []
    for cname, py in structs:
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        expect.append(C.sizeof(py))
        for fld in py._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {fld[0]}));')
            expect.append(getattr(py, fld[0]).offset)
    lines.append('printf("%d %d %d %d %d\\n", CTL_BSDF_DIELECTRIC, CTL_BSDF_THINDIELECTRIC, CTL_BSDF_CONDUCTOR, '
                 'CTL_BSDF_ROUGHCONDUCTOR, CTL_BSDF_PLASTIC);')
    lines.append('printf("%d %d %d\\n", CTL_ENULL, CTL_EDELTA_REFLECTION, CTL_EDELTA_TRANSMISSION);')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == expect + [3, 4, 6, 7, 8, 0x1, 0x20, 0x40]
    # the ext array is the desc's last member: code built against the shorter desc reads what it knew
    assert _abi.SceneDesc.materials_ext.offset + 8 == C.sizeof(_abi.SceneDesc)


def _quad_scene(mats_per_mesh):
    hs = ctl.HostScene()
    for k, mats in enumerate(mats_per_mesh):
        v = np.array(BC.QUAD_V, np.float32) + np.float32(3 * k)
        hs.add_node(hs.add_mesh(v, BC.QUAD_I, mats, mat_index=[0, len(mats) - 1]))
    hs.set_camera((0, 3, 0.01), (0, 0, 0), (0, 1, 0), 40.0, 32, 32)
    return hs


def test_host_compile_lays_ext_out_parallel_to_materials():
    gold = ctl.conductor_material(BC.GOLD_ETA, BC.GOLD_K)
    pl = ctl.plastic_material(1.5, (0.5, 0.3, 0.2))
    hs = _quad_scene([[ctl.diffuse_material(0.5, 0.5, 0.5), ctl.dielectric_material(1.5)],   # no ext records
                      [gold, ctl.diffuse_material(0.1, 0.2, 0.3), pl],
                      [ctl.thindielectric_material(1.5)]])
    d = hs.compile()
    assert d.n_materials == 6 and d.materials_ext
    types = [d.materials[i].bsdf_type for i in range(6)]
    assert types == [1, 3, 6, 1, 8, 4]
    ext = [d.materials_ext[i] for i in range(6)]
    for i in (0, 1, 3, 5):
        assert bytes(ext[i]) == bytes(64)
    assert list(ext[2].eta) == [np.float32(x) for x in BC.GOLD_ETA] and list(ext[2].k) == [np.float32(x) for x in BC.GOLD_K]
    assert ext[4].fdr_int == pl[1].fdr_int and ext[4].inv_eta2 == pl[1].inv_eta2
    assert 0.0 < ext[4].specular_sampling_weight < 1.0
    # no ext record anywhere: no array
    d2 = _quad_scene([[ctl.diffuse_material(0.5, 0.5, 0.5), ctl.dielectric_material(1.5)]]).compile()
    assert not d2.materials_ext
    # a wrong count is refused
    L = ctl.lib()
    e = (_abi.MaterialExt * 1)()
    assert L.ctl_host_scene_set_mesh_material_ext(hs._h, 1, e, 1) != 0
    assert b"ext" in L.ctl_host_last_error()


def test_plastic_update_members():
    """plastic::Update(): m_invEta2, m_fdrInt by the Gauss-Lobatto quadrature, the sampling weight."""
    m, e = ctl.plastic_material(1.5, (0.5, 0.5, 0.5), (1.0, 1.0, 1.0))
    assert e.inv_eta2 == np.float32(1.0) / (np.float32(1.5) * np.float32(1.5))
    # the internal diffuse Fresnel reflectance of eta = 1.5 is 0.5963 (Egan & Hilgeman's fit: 0.5965)
    assert abs(e.fdr_int - 0.5963) < 2e-3
    fit = -1.4399 * (1 / 1.5) ** 2 + 0.7099 / 1.5 + 0.6681 + 0.0636 * 1.5
    assert abs(e.fdr_int - fit) < 2e-3
    assert abs(e.specular_sampling_weight - 1.0 / 1.5) < 1e-6
    assert abs(float(ctl.fresnel_diffuse_reflectance(1.5)) - 0.0918) < 2e-3   # external, d'Eon & Irving: 0.0918


def test_xmsh_round_trip_of_types_3_and_4_and_refusal_of_6_to_8():
    mats = [ctl.dielectric_material(1.5, (0.9, 0.8, 0.7), (0.6, 0.7, 0.95)), ctl.thindielectric_material(1.3, two_sided=True)]
    hs = _quad_scene([mats])
    hs.compile()
    data = hs.write_xmsh(0)
    hs2 = ctl.HostScene()
    hs2.add_node(hs2.add_xmsh(data))
    hs2.set_camera((0, 3, 0.01), (0, 0, 0), (0, 1, 0), 40.0, 32, 32)
    d2 = hs2.compile()
    assert d2.n_materials == 2
    for i in range(2):
        assert bytes(d2.materials[i]) == bytes(hs.desc.materials[i])
        assert d2.materials[i].bsdf_type == mats[i].bsdf_type and d2.materials[i].eta == mats[i].eta
        assert list(d2.materials[i].transmittance) == list(mats[i].transmittance)
    for bad in (ctl.conductor_material(BC.GOLD_ETA, BC.GOLD_K), ctl.roughconductor_material(1, BC.GOLD_ETA, BC.GOLD_K, 0.3),
                ctl.plastic_material(1.5)):
        hs3 = _quad_scene([[ctl.diffuse_material(0.5, 0.5, 0.5), bad]])
        hs3.compile()
        with pytest.raises(ctl.CTLError, match="ctl_material_ext"):
            hs3.write_xmsh(0)


def test_scene_cache_round_trip_with_the_ext_array(tmp_path):
    _, desc = BC.host_scene()
    path = str(tmp_path / "scene.bin")
    scene_cache.save(desc, path)
    c = scene_cache.load(path)
    try:
        n = desc.n_materials
        assert c.desc.n_materials == n and c.desc.materials_ext
        assert C.string_at(c.desc.materials_ext, 64 * n) == C.string_at(desc.materials_ext, 64 * n)
        assert C.string_at(c.desc.materials, 80 * n) == C.string_at(desc.materials, 80 * n)
        q = BC.delta_queries(R.CONDUCTOR)[:500]
        assert BC.same_bits(ctl.host_bsdf_eval(c.desc, q), ctl.host_bsdf_eval(desc, q)).size == 0
    finally:
        c.close()


def test_host_entry_refuses_what_upload_refuses():
    hs = _quad_scene([[ctl.conductor_material(BC.GOLD_ETA, BC.GOLD_K)[0]]])   # the ext record left out
    d = hs.compile()
    with pytest.raises(ctl.CTLError, match="ctl_material_ext"):
        ctl.host_bsdf_eval(d, np.zeros(1, dtype=ctl.BSDF_QUERY_DTYPE))
    # a material index past the array: no read, a marked result
    q = np.zeros(1, dtype=ctl.BSDF_QUERY_DTYPE)
    q[0]["material"] = 10 ** 6
    assert int(_eval(q)[0]["sampled_type"]) == 0xFFFFFFFF
