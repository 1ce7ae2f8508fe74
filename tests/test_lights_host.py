"""Point, spot and distant lights on the CPU: the records the scene compiler emits and what it refuses,
the host evaluator (ctl_host_light_eval) against a float64 statement of Light::sampleDirect
(light_ref.py), and edge queries with exact expectations."""
import numpy as np
import pytest

import light_cases as LC
import light_ref as LR

A = None


@pytest.fixture(scope="module", autouse=True)
def _abi(ctl):
    global A
    A = ctl._abi


# ---------------------------------------------------------------------------------------------
def test_records_of_the_mixed_scene(ctl):
    """One area light, the environment and one light of each new kind: kinds, order, slots, the light
    CDF and env_map_index; and the scene without the three compiles to the same bytes as before the
    adds (every array and every scalar of the description)."""
    s, _ = LC.mixed_host_scene(ctl, delta=False)
    before = LC.desc_bytes(ctl, s.compile())
    n_tris_before = s.desc.n_light_tris
    assert [s.desc.lights[i].kind for i in range(s.desc.n_lights)] == [A.CTL_LIGHT_DIFFUSE, A.CTL_LIGHT_INFINITE]
    idx = LC.add_mixed_delta_lights(s)
    assert idx == [2, 3, 4]
    d = s.compile()
    assert d.n_lights == 5 and d.env_map_index == 1
    assert [d.lights[i].kind for i in range(5)] == [A.CTL_LIGHT_DIFFUSE, A.CTL_LIGHT_INFINITE, A.CTL_LIGHT_POINT,
                                                    A.CTL_LIGHT_SPOT, A.CTL_LIGHT_DISTANT]
    assert d.n_light_tris == n_tris_before + 3
    cdf = np.array(d.light_cdf[:], np.float32)
    step = np.float32(1.0) / np.float32(5.0)
    want = np.cumsum(np.full(5, step, np.float32), dtype=np.float32)
    assert np.array_equal(cdf[:5], want) and not cdf[5:].any()
    for k, i in enumerate(idx):
        L = d.lights[i]
        assert (L.node_idx, L.tri_count, L.tri_first, L.orthogonal) == (0xFFFFFFFF, 0, n_tris_before + k, 0)
    # the slots: what the reference's constructors compute, from the fp32 inputs
    P = LC.light_slot(d, 2)
    assert np.array_equal(np.array(P.pos[:], np.float32), LC.MIXED_POINT["pos"])
    assert not any(P.s[:] + P.t[:] + P.n[:]) and P.cos_beam_width == P.cos_cutoff_angle == P.cutoff_angle == 0
    assert np.array_equal(np.array(d.lights[2].radiance[:], np.float32), LC.MIXED_POINT["I"])
    sp = LC.MIXED_SPOT
    P = LC.light_slot(d, 3)
    axis = sp["target"].astype(np.float64) - sp["pos"]
    axis /= np.linalg.norm(axis)
    frame = np.array([P.s[:], P.t[:], P.n[:]], np.float64)
    assert np.abs(frame[2] - axis).max() < 2e-7
    assert np.abs(frame @ frame.T - np.eye(3)).max() < 5e-7 and np.linalg.det(frame) > 0.99
    cutoff, beam = np.float32(np.pi) / np.float32(180) * sp["cutoff"], np.float32(np.pi) / np.float32(180) * sp["beam"]
    assert P.cutoff_angle == cutoff and P.inv_transition_width == np.float32(1) / (cutoff - beam)
    assert P.cos_cutoff_angle == np.float32(np.cos(np.float64(cutoff))) and P.cos_beam_width == np.float32(np.cos(np.float64(beam)))
    ds = LC.MIXED_DISTANT
    P = LC.light_slot(d, 4)
    n = ds["dir"].astype(np.float64) / np.linalg.norm(ds["dir"].astype(np.float64))
    assert np.abs(np.array(P.n[:]) - n).max() < 2e-7 and P.cos_beam_width == ds["r"] * np.float32(1.1)
    assert not any(P.pos[:]) and P.cos_cutoff_angle == P.cutoff_angle == P.inv_transition_width == 0
    # everything the area light and the environment own is where it was
    after = LC.desc_bytes(ctl, d)
    changed = {k for k in before if before[k] != after[k]}
    assert changed <= {"lights", "n_lights", "light_tris", "n_light_tris", "light_cdf"}, changed
    assert after["lights"][:len(before["lights"])] == before["lights"]
    assert after["light_tris"][:len(before["light_tris"])] == before["light_tris"]
    # and a scene that never saw the adds compiles to the bytes of the compile made before them
    s2, _ = LC.mixed_host_scene(ctl, delta=False)
    again = LC.desc_bytes(ctl, s2.compile())
    assert {k for k in before if before[k] != again[k]} == set()


def test_compiler_refusals(ctl):
    inf, nan = float("inf"), float("nan")
    s, _ = LC.mixed_host_scene(ctl, delta=False)
    ok3 = (1.0, 2.0, 3.0)
    cases = [
        (lambda: s.add_point_light((0, nan, 0), ok3), "non-finite"),
        (lambda: s.add_point_light((0, 0, 0), (1, inf, 1)), "non-finite"),
        (lambda: s.add_spot_light((0, 1, 0), (0, 1, 0), ok3, 40, 20), "target"),
        (lambda: s.add_spot_light((0, 1, 0), (0, 0, 0), ok3, 20, 40), "beam"),
        (lambda: s.add_spot_light((0, 1, 0), (0, 0, 0), ok3, nan, 20), "non-finite"),
        (lambda: s.add_spot_light((0, 1, 0), (inf, 0, 0), ok3, 40, 20), "non-finite"),
        (lambda: s.add_distant_light(ok3, (0, 0, 0), 1.0), "zero"),
        (lambda: s.add_distant_light(ok3, (0, 1, 0), inf), "non-finite"),
        (lambda: s.add_distant_light((1, nan, 1), (0, 1, 0), 1.0), "non-finite"),
    ]
    for f, match in cases:
        with pytest.raises(ctl.CTLError, match=match):
            f()
    # equal spot angles are legal (the loader's sun: 90 / 90)
    first = s.add_spot_light((0, 1, 0), (0, 0, 0), ok3, 90, 90)
    assert first == 2                                     # after the area light and the environment
    for k in range(13):
        assert s.add_point_light((k, 1, 0), ok3) == 3 + k
    for add in (lambda: s.add_point_light((0, 1, 0), ok3), lambda: s.add_spot_light((0, 1, 0), (0, 0, 0), ok3, 40, 20),
                lambda: s.add_distant_light(ok3, (0, 1, 0), 1.0)):
        with pytest.raises(ctl.CTLError, match="16"):
            add()
    d = s.compile()
    assert d.n_lights == 16
    assert np.isposinf(LC.light_slot(d, 2).inv_transition_width)
    cdf = np.array(d.light_cdf[:], np.float32)
    assert np.all(np.diff(cdf) > 0) and abs(cdf[-1] - 1.0) < 1e-6


def test_host_evaluator_refuses_a_damaged_description(ctl):
    s, d = LC.eval_scene(ctl)
    q = LC.queries(ctl, 0, [[0, 0, 0]])
    L = d.lights[LC.I_SPOT0]
    keep = L.tri_first
    try:
        L.tri_first = d.n_light_tris
        with pytest.raises(ctl.CTLError, match="slot"):
            ctl.host_light_eval(d, q)
    finally:
        L.tri_first = keep
    r = ctl.host_light_eval(d, LC.queries(ctl, 99, [[0, 0, 0]]))
    assert r["measure"][0] == 0xFFFFFFFF and not r["value"].any()


# ---------------------------------------------------------------------------------------------
# Tolerances of the random sets (the issue's, with their derivations).
#
# REL = 1e-5 for value, d, dist and p of the point and distant lights and of the spot outside its
# transition band: each result is reached in under 20 fp32 roundings of 2^-24 = 6e-8 each; the one
# cancelling step, p - ref, amplifies the error of its inputs by at most 16, because the reference
# points are drawn with |p - ref| >= max(|p|, |ref|) / 8, and only the one or two roundings in front
# of it are amplified: 2 * 6e-8 * 16 + 18 * 6e-8 = 3e-6, with headroom.  Vectors are compared in
# norm, relative to the vector's norm.
#
# BAND = 4e-6 * inv_transition_width, absolute, on the falloff factor inside the band: cosTheta
# carries at most 4 ulp of 6e-8 (d's roundings and the dot product), which acos turns into an angle
# error of at most 2.4e-7 / sin(theta).  Cutoff angles are >= 10 degrees and transition widths >= 2
# degrees; the narrowest spot here (10 / 8 degrees) has its band at theta >= 8 degrees, where that is
# 1.7e-6, and at sin(10 deg) it is 1.4e-6.  cutoff_angle's own rounding (<= 8e-8 at 75 degrees) and
# acos's (<= 8e-8) add 1.6e-7.  4e-6 leaves room for the frame's rounding: the axis comes from
# target - pos, a subtraction the spots here condition by at most 4.
REL = 1e-5
BAND = 4e-6
COS_EXCLUDE = 1e-6      # |cosTheta - threshold| below which fp32 may take the other branch
DIST_EXCLUDE = 1e-5     # |distance| / radius below which the distant light's branch may go either way
MAX_EXCLUDED = 0.01


def _rel_vec(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)


def check_random_set(name, q, got, ref):
    n = q.shape[0]
    assert n == 4096
    keep = np.ones(n, bool)
    band = np.zeros(n, bool)
    spot = None
    if name.startswith("spot"):
        spot = LC.SPOTS[int(name[4:])]
        assert spot["cutoff"] >= 10 and spot["cutoff"] - spot["beam"] >= 2
        cc, cb = np.cos(np.radians(np.float64(spot["cutoff"]))), np.cos(np.radians(np.float64(spot["beam"])))
        keep &= (np.abs(ref["cos_theta"] - cc) > COS_EXCLUDE) & (np.abs(ref["cos_theta"] - cb) > COS_EXCLUDE)
        band = (ref["cos_theta"] > cc) & (ref["cos_theta"] < cb)
        # the draw reaches all three regions
        assert min(band.sum(), (ref["cos_theta"] >= cb).sum(), (ref["cos_theta"] <= cc).sum()) > n // 20, name
    if name == "distant":
        keep &= np.abs(ref["distance"]) > DIST_EXCLUDE * ref["radius"]
        assert (~ref["lit"]).sum() > n // 20 and ref["lit"].sum() > n // 4
    assert (~keep).sum() <= MAX_EXCLUDED * n, (name, int((~keep).sum()))
    lit = keep & (ref["pdf"] > 0)
    dark = keep & (ref["pdf"] == 0)            # the distant light's points behind the disk
    assert np.all(got["pdf"][lit] == 1.0) and np.all(got["measure"][lit] == LR.DISCRETE), name
    assert not got["value"][dark].any() and not got["pdf"][dark].any(), name
    worst = {}
    worst["d"] = _rel_vec(got["d"][lit], ref["d"][lit]).max()
    worst["dist"] = (np.abs(got["dist"][lit] - ref["dist"][lit]) / ref["dist"][lit]).max()
    if name == "distant":
        worst["p"] = _rel_vec(got["p"][lit], ref["p"][lit]).max()
        assert np.abs(got["n"][lit] + got["d"][lit]).max() == 0
    else:
        assert np.array_equal(got["p"][lit], np.broadcast_to(ref["p"][0].astype(np.float32), got["p"][lit].shape))
        assert not got["n"][lit].any()
    flat = lit & ~band
    v, w = got["value"][flat].astype(np.float64), ref["value"][flat]
    nz = w != 0
    assert not v[~nz].any(), name                         # outside the cutoff: exactly 0
    worst["value"] = (np.abs(v[nz] - w[nz]) / w[nz]).max()
    print(f"{name}: worst relative errors {worst}, excluded {int((~keep).sum())}")
    assert all(e <= REL for e in worst.values()), (name, worst)
    if spot is not None:
        b = lit & band
        itw = 1.0 / (np.radians(np.float64(spot["cutoff"])) - np.radians(np.float64(spot["beam"])))
        # the falloff factor's absolute tolerance scaled by the value's other factors (I / dist^2), plus
        # the relative tolerance those factors have on their own
        tol = BAND * itw * ref["unattenuated"][b] + REL * ref["value"][b]
        err = np.abs(got["value"][b].astype(np.float64) - ref["value"][b])
        print(f"{name}: band worst error / tolerance {(err / tol).max():.3f} over {int(b.sum())} queries")
        assert np.all(err <= tol), (name, float((err / tol).max()))


def test_host_evaluator_against_float64(ctl):
    _, d = LC.eval_scene(ctl)
    for name, q, ref in LC.random_sets(ctl):
        check_random_set(name, q, ctl.host_light_eval(d, q), ref)


# ---------------------------------------------------------------------------------------------
def test_edge_queries_on_the_host(ctl):
    _, d = LC.edge_scene(ctl)
    sets = LC.edge_sets(ctl)
    f = np.float32
    P = LC.light_slot(d, LC.E_SPOT)
    I = LC.EDGE_SPOT["I"]
    # cosTheta == cos_cutoff_angle exactly: `<=` puts it outside, value 0 (the record is still filled)
    r = ctl.host_light_eval(d, sets["spot_at_cutoff"])
    assert np.all(-r["d"][:, 2] == f(P.cos_cutoff_angle))
    assert not r["value"].any() and np.all(r["pdf"] == 1) and np.all(r["measure"] == LR.DISCRETE)
    # cosTheta == cos_beam_width exactly: `>=` puts it on the plateau, value I / dist^2 with no falloff
    r = ctl.host_light_eval(d, sets["spot_at_beam"])
    assert np.all(-r["d"][:, 2] == f(P.cos_beam_width))
    inv = f(1) / r["dist"]
    assert np.array_equal(r["value"], I[None, :] * (inv * inv)[:, None])
    # the distant light: a point on the disk's plane is lit from distance 0, one behind it gets nothing
    E = LC.EDGE_DISTANT["E"]
    r = ctl.host_light_eval(d, sets["distant_on_plane"])
    assert np.all(r["dist"] == 0) and np.array_equal(r["value"], np.tile(E, (2, 1))) and np.all(r["pdf"] == 1)
    assert np.array_equal(r["p"], sets["distant_on_plane"]["ref"]) and np.all(r["measure"] == LR.DISCRETE)
    assert np.array_equal(r["d"], np.tile(f([0, 0, -1]), (2, 1))) and np.array_equal(r["n"], np.tile(f([0, 0, 1]), (2, 1)))
    r = ctl.host_light_eval(d, sets["distant_behind"])
    assert not r["value"].any() and not r["pdf"].any()
    # equal angles: inv_transition_width is +inf and never read: every value is 0 or I / dist^2
    for k in range(2):
        assert np.isposinf(LC.light_slot(d, LC.E_EQ0 + k).inv_transition_width)
        q = sets[f"equal_angles{k}"]
        r = ctl.host_light_eval(d, q)
        assert np.isfinite(r["value"]).all()
        inv = f(1) / r["dist"]
        full = LC.EDGE_EQ[k]["I"][None, :] * (inv * inv)[:, None]
        inside = -r["d"][:, 2] > f(LC.light_slot(d, LC.E_EQ0 + k).cos_cutoff_angle)
        assert inside.any() and (~inside).any()
        assert np.array_equal(r["value"], np.where(inside[:, None], full, f(0)))
    # ref == pos: the reference divides by zero; the restatement gives dist 0 and a direction of NaNs
    r = ctl.host_light_eval(d, sets["ref_is_pos"])
    assert np.all(r["dist"] == 0) and np.isnan(r["d"]).all()
    assert np.isposinf(r["value"][0]).all()
