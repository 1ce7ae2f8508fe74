"""The oracle's restatement of dielectric, thindielectric, conductor, roughconductor and plastic
(oracle/oracle_mat.h), checked without a GPU: its BSDF answers against the product's host entry and
against the numpy restatement, the three closed-form renders applied to its images, its refusal of
what it does not restate, and the event counts that show scenes A and B reach the branches the GPU
tests (test_gpu_materials_oracle.py) are there for."""
import ctypes as C

import numpy as np
import pytest

import bsdf_cases as BC
import bsdf_ref as R
import materials_scenes as MS
import oracle
from helpers import binary_bvh, oracle_render, tie_rule


def _report(q, got, want, bad):
    i = int(bad[0])
    return f"{len(bad)} of {len(q)} queries differ; first: query {q[i]} got {got[i]} want {want[i]}"


def _queries(type):
    return BC.roughconductor_queries() if type == R.ROUGHCONDUCTOR else BC.delta_queries(type)


def _oracle_eval(q):
    return oracle.bsdf_eval(BC.host_scene()[1], q)


@pytest.mark.parametrize("type", [R.DIELECTRIC, R.THINDIELECTRIC, R.CONDUCTOR, R.PLASTIC, R.ROUGHCONDUCTOR])
def test_oracle_bsdf_eval_equals_the_host_entry_bit_for_bit(ctl, type):
    """oracle_bsdf_eval (written from the reference) against ctl_host_bsdf_eval (the product's dispatch
    on the CPU) on the project's query sets; test_batch_entry_equals_the_host_entry_bit_for_bit
    carries the result on to the device."""
    q = _queries(type)
    assert len(q) >= 4000
    if type == R.ROUGHCONDUCTOR:   # the anisotropic and the two-sided materials are in the set
        assert set(np.unique(q["material"])) == set(BC.indices_of(R.ROUGHCONDUCTOR, appended=True))
        assert len(BC.indices_of(R.ROUGHCONDUCTOR, appended=True)) == 5
    got, want = _oracle_eval(q), ctl.host_bsdf_eval(BC.host_scene()[1], q)
    bad = BC.same_bits(got, want)
    assert bad.size == 0, _report(q, got, want, bad)
    assert (want["value"].max(axis=1) > 0).sum() > len(q) // 20


def test_appended_materials_left_the_indices_alone():
    A, D = BC.materials()
    assert len(A) == 21 and not any(d and d.get("appended") for d in D[:18]) and all(d.get("appended") for d in D[18:])
    assert BC.indices_of(R.ROUGHCONDUCTOR) == [14, 15] and BC.indices_of(5) == [16, 17]
    m = [A[i][0] for i in BC.indices_of(R.ROUGHCONDUCTOR, appended=True)[2:]]
    assert all(x.alpha_u != x.alpha_v for x in m)
    assert {x.distribution for x in m[:2]} == {0, 1} and [x.two_sided for x in m] == [0, 0, 1]


@pytest.mark.parametrize("type", [R.DIELECTRIC, R.THINDIELECTRIC, R.CONDUCTOR])
def test_oracle_delta_types_match_the_numpy_restatement(type):
    q = BC.delta_queries(type)
    got, want = _oracle_eval(q), BC.reference(q)
    bad = BC.same_bits(got, want)
    assert bad.size == 0, _report(q, got, want, bad)


def test_oracle_plastic_matches_the_numpy_restatement():
    """The warp table comes from the oracle's own diffuse material, so nothing of the product is in
    this comparison."""
    q = BC.delta_queries(R.PLASTIC)
    got = _oracle_eval(q)
    want, n_warps = BC.plastic_reference(q, _oracle_eval)
    assert n_warps >= 50 and (want["sampled_type"] == R.EDIFFUSE_REFLECTION).sum() >= 300
    bad = BC.same_bits(got, want)
    assert bad.size == 0, _report(q, got, want, bad)


# ---------------------------------------------------------------------------------------------
# the closed-form renders, judged on the oracle's images
@pytest.mark.parametrize("direct", [1, 0])
def test_oracle_invisible_panes(ctl, orc, direct):
    w, h, passes = 32, 32, 4
    s, d = MS.invisible_panes_scene(ctl, w, h)   # the host scenes own the descs' arrays
    p = ctl.PTParams(direct, 50, 5, 1, 64, 1, 0, 0)
    got, _ = oracle_render(orc, d, p, passes, w, h)
    s0, d0 = MS.env_only(ctl, w, h, MS.PANES_CAM)
    want, _ = oracle_render(orc, d0, p, passes, w, h)
    MS.check_invisible_panes(got, want, passes, f"oracle, direct {direct}")


def test_oracle_mirror_wall(ctl, orc):
    w, h = 32, 32
    s, d = MS.mirror_wall_scene(ctl, w, h)
    p = ctl.PTParams(0, 2, 5, 1, 64, 1, 0, 0)
    got, _ = oracle_render(orc, d, p, 1, w, h)
    s0, d0 = MS.env_only(ctl, w, h, MS.MIRROR_CAM)
    env, _ = oracle_render(orc, d0, p, 1, w, h)
    MS.check_mirror_wall(orc, got, env, d, w, h)


@pytest.mark.parametrize("nonlinear", [False, True])
def test_oracle_textured_plastic_equals_constant_plastic(ctl, orc, nonlinear):
    p = ctl.PTParams(1, 6, 3, 1, 64, 1, 0, 0)
    (s1, d1), (s2, d2) = MS.textured_plastic_scene(ctl, nonlinear, True), MS.textured_plastic_scene(ctl, nonlinear, False)
    a, _ = oracle_render(orc, d1, p, 3, 32, 32)
    b, _ = oracle_render(orc, d2, p, 3, 32, 32)
    MS.check_textured_plastic(a, b)


# ---------------------------------------------------------------------------------------------
# what the oracle does not restate, it refuses
def _one_material(ctl, mat):
    s = ctl.HostScene()
    m = MS.Mesh()
    m.quad([(-1, 0, -1), (-1, 0, 1), (1, 0, 1), (1, 0, -1)], 0)
    s.add_node(m.add_to(s, [mat]))
    s.set_camera((0, 3, 0.01), (0, 0, 0), (0, 1, 0), 40.0, 8, 8)
    return s, s.compile()


def _shading_entries(ctl, orc, d):
    """Every oracle entry that shades, as a callable on the desc."""
    n = d.camera.width * d.camera.height
    fb, depth, ev = np.zeros((n, 7), np.float32), np.zeros(n, np.float32), np.zeros(7, np.uint64)
    p = ctl.PTParams(1, 4, 3, 1, 16, 1, 0, 0)
    pp = ctl.PrimParams(ctl._abi.PRIM_DRAW_MODES.index("first_f"), 7, 1.0, 100.0, 0)
    q = np.zeros(1, dtype=ctl.BSDF_QUERY_DTYPE)
    return {"oracle_render_pass": lambda: orc.oracle_render_pass(C.byref(d), C.byref(p), 0, oracle.ptr(fb), 0, 1, 1, None),
            "oracle_render_pass_events": lambda: orc.oracle_render_pass_events(C.byref(d), C.byref(p), 0, oracle.ptr(fb), 0,
                                                                               1, oracle.ptr(ev)),
            "oracle_wpt_render_pass": lambda: orc.oracle_wpt_render_pass(C.byref(d), 1, 4, 3, 1, 0, oracle.ptr(fb), 0, 1),
            "oracle_prim_pass": lambda: orc.oracle_prim_pass(C.byref(d), C.byref(pp), 0, oracle.ptr(fb), oracle.ptr(depth), 0,
                                                             1),
            "oracle_bsdf_eval": lambda: oracle.bsdf_eval(d, q),
            "helpers.oracle_render": lambda: oracle_render(orc, binary_bvh(d), p, 1, d.camera.width, d.camera.height)}, fb


@pytest.mark.parametrize("bsdf_type", [2, 9, 10, 11, 12, 13, 14, 15, 0, 16])
def test_oracle_refuses_types_it_does_not_restate(ctl, orc, bsdf_type):
    s, d = _one_material(ctl, ctl.diffuse_material(0.5, 0.5, 0.5))
    entries, fb = _shading_entries(ctl, orc, d)
    assert set(oracle.SHADING_ENTRIES) <= set(entries)
    for call in entries.values():   # well-formed: every entry runs
        call()
    d.materials[0].bsdf_type = bsdf_type
    fb[:] = 0
    for name, call in entries.items():
        with pytest.raises(oracle.OracleError, match=f"material 0 .bsdf_type {bsdf_type}.*not restated"):
            call()
    assert not fb.any()   # nothing was rendered: no guess


@pytest.mark.parametrize("make", ["conductor", "roughconductor", "plastic"])
def test_oracle_refuses_types_6_7_8_without_ext(ctl, orc, make):
    gold = (BC.GOLD_ETA, BC.GOLD_K)
    mat = {"conductor": lambda: ctl.conductor_material(*gold), "roughconductor": lambda: ctl.roughconductor_material(1, *gold, 0.3),
           "plastic": lambda: ctl.plastic_material(1.5)}[make]()
    s, d = _one_material(ctl, mat)
    entries, fb = _shading_entries(ctl, orc, d)
    for call in entries.values():
        call()
    d.materials_ext = None
    fb[:] = 0
    for name, call in entries.items():
        with pytest.raises(oracle.OracleError, match="material 0 .*ctl_material_ext"):
            call()
    assert not fb.any()


def test_oracle_refuses_the_sampling_it_does_not_restate(ctl, orc):
    s, d = _one_material(ctl, ctl.roughconductor_material(1, BC.GOLD_ETA, BC.GOLD_K, 0.3))
    entries, _ = _shading_entries(ctl, orc, d)
    d.materials[0].sample_visible = 0
    for call in entries.values():
        with pytest.raises(oracle.OracleError, match="visible-normal"):
            call()
    # the first_non_delta draw modes on a scene with a delta material: the product refuses them too
    _, d = MS.scene("A")
    fb, depth = np.zeros((MS.W * MS.H, 7), np.float32), np.zeros(MS.W * MS.H, np.float32)
    for mode in (12, 13, 14):
        pp = ctl.PrimParams(mode, 7, 1.0, 100.0, 0)
        with pytest.raises(oracle.OracleError, match="first_non_delta"):
            orc.oracle_prim_pass(C.byref(d), C.byref(pp), 0, oracle.ptr(fb), oracle.ptr(depth), tie_rule(d, orc), 1)


# ---------------------------------------------------------------------------------------------
# the scenes reach what they are there for
@pytest.mark.parametrize("direct", [1, 0])
@pytest.mark.parametrize("name,render", sorted(MS.EVENTS_OF))
def test_event_floors(name, render, direct):
    """A condition on the inputs of the GPU tests, not a measurement: every render of scene A and B
    that they compare goes through each branch it is listed for at least 50 times, by the oracle's
    own counters.  A scene that falls short is changed, not the floor."""
    fb, rays, events = MS.reference(name, direct, "wide", render)
    print(f"scene {name}, render {render} {MS.RENDERS[render]}, direct {direct}: {rays} rays, {events}")
    for e in MS.EVENTS_OF[(name, render)]:
        if e == "nee_on_delta_and_smooth" and not direct:
            assert events[e] == 0
            continue
        assert events[e] >= MS.EVENT_FLOOR, (e, events)
    assert np.isfinite(fb).all() and fb[:, :3].max() > 0 and (fb[:, 6] > 0).sum() > 0.9 * MS.W * MS.H


def test_scene_b_is_laid_out_as_the_tests_need(ctl):
    """Two meshes under two nodes, the second node transformed and its materials behind an offset, its
    ext records behind mesh 0's; the glass is one-sided with R != T != 1, the plastic's reflectance a
    non-constant bilinear texture, one rough conductor anisotropic GGX and one Beckmann."""
    _, d = MS.scene("B")
    assert d.n_nodes == 2 and d.n_meshes == 2 and d.nodes[0].material_offset == 0 and d.nodes[1].material_offset == 3
    m = [d.materials[i] for i in range(d.n_materials)]
    assert [x.bsdf_type for x in m] == [1, 1, 3, 6, 8, 7, 7, 4]
    glass = m[2]
    assert not glass.two_sided and glass.eta == 1.5 and list(glass.reflectance) != list(glass.transmittance)
    assert 1.0 not in list(glass.reflectance) + list(glass.transmittance)
    assert m[4].texture != 0xFFFFFFFF and d.materials_ext[4].nonlinear == 1
    t = d.textures[m[4].texture]
    assert t.filter == ctl._abi.CTL_TEX_BILINEAR
    texels = np.ctypeslib.as_array(d.tex_data, shape=(t.offsets[0] + t.width * t.height,))[t.offsets[0]:]
    assert len(np.unique(texels)) > 8
    assert m[5].distribution == 1 and m[5].alpha_u != m[5].alpha_v and m[6].distribution == 0
    assert m[7].two_sided and list(d.materials_ext[3].eta) == [np.float32(x) for x in BC.GOLD_ETA]
    xf = np.array(d.node_xf[1].m[:]).reshape(4, 4)
    assert xf[0, 2] != 0 and xf[2, 0] == -xf[0, 2] and xf[0, 3] != 0 and np.array_equal(xf[1], [0, 1, 0, 0])   # turned about y, moved
    assert np.array_equal(np.array(d.node_xf[0].m[:]).reshape(4, 4), np.eye(4))
