"""The five sensors on the CPU: the host evaluator (ctl_host_sensor_eval) against a float64 statement of
Sensor::sampleRay and Sensor::sampleRayDifferential (sensor_ref.py), the closed forms each type obeys, what
the scene compiler and the evaluator refuse, and the ABI's record sizes."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import sensor_cases as SC
import sensor_ref as SR
from helpers import camera_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---------------------------------------------------------------------------------------------
# Tolerances, from the count of fp32 roundings in each type's formula (each at most EPS = 2^-24 of the value it
# rounds).  K[type] roundings bound the absolute error of a direction (a unit vector: every intermediate is no
# larger than the vector it ends in) and, relative to SCALE = |toWorld's translation| + |the camera-space point|
# (the size of the terms summed), that of an origin.  The pieces:
#   P  x * invResolution 1 + m_sampleToCamera.TransformPoint 8 (4 products, 3 sums, the division by w) = 9
#   N  normalize 8 (3 squares, 2 sums, sqrt, rcp, the product)
#   D  toWorld.TransformDirection 5 (3 products, 2 sums);  T  toWorld.TransformPoint 8
#   L  the lens point 8: 2 u - 1 2, the ratio and its product with pi / 4 3, sin or cos 1, r * 1, the radius 1
#   X  rayX / rayY: one more sum (nearP + m_dx, orig + m_dx)
#   perspective   direction P + X + N + D = 23; the origin is Translation() itself
#   thin lens     direction P + X + the focal scale f / nearP.z and its product 2 + minus the lens point 1 + L + N
#                 + D = 34; origin L + T = 16
#   orthographic  the direction is Forward(): exact; origin P + X + T = 18
#   telecentric   origin L + P + their sum 1 + X + T = 27; direction: focusP - orig 1 on P and L, then D and N: 32
#   spherical     the angle (1 - x inv) * 2 * pi carries 3 roundings at a magnitude of up to 2 pi: 3 * 2 pi = 19, then
#                 sin / cos 1, the product 1 and D 5: 26
# The float64 statement's own error is far below one EPS.
EPS = 2.0 ** -24
K = {"perspective": 23, "thinlens": 34, "orthographic": 18, "telecentric": 32, "spherical": 26}


def _scale(desc, ref_o):
    t = np.array([desc.camera.to_world.m[3], desc.camera.to_world.m[7], desc.camera.to_world.m[11]], np.float64)
    return np.linalg.norm(t) + np.linalg.norm(ref_o - t, axis=1)


def check_against_reference(name, desc, q, got, k):
    ref = SC.ref_rays(desc, q)
    worst = 0.0
    scale = _scale(desc, ref[0])
    for field, want, rel in (("o", ref[0], scale), ("d", ref[1], 1.0), ("ox", ref[2], scale), ("dx", ref[3], 1.0),
                             ("oy", ref[4], scale), ("dy", ref[5], 1.0)):
        if want is None:
            assert not got[field].any(), (name, field)
            continue
        err = np.linalg.norm(got[field].astype(np.float64) - want, axis=1) / rel
        worst = max(worst, float(err.max()))
    defined = ref[2] is not None
    assert np.all(got["has_differentials"] == (1 if defined else 0)), name
    print(f"{name}: worst error / tolerance {worst / (k * EPS):.3f}")
    assert worst <= k * EPS, (name, worst / (k * EPS))


@pytest.fixture(scope="module")
def scenes(ctl):
    return {kind: SC.quad_scene(ctl, kind) for kind in SC.KINDS}


@pytest.mark.parametrize("differential", [False, True])
@pytest.mark.parametrize("kind", SC.KINDS)
def test_host_evaluator_against_the_float64_statement(ctl, scenes, kind, differential):
    _, d = scenes[kind]
    assert d.sensor and d.sensor[0].type == SR.KINDS[kind]
    for what, q in (("random", SC.random_queries(ctl, differential)), ("edges", SC.edge_queries(ctl, differential))):
        got = ctl.host_sensor_eval(d, q)
        assert np.isfinite(got["o"]).all() and np.isfinite(got["d"]).all()
        check_against_reference(f"{kind} {'sampleRayDifferential' if differential else 'sampleRay'} {what}", d, q, got, K[kind])


def test_perspective_equals_the_camera_rays_helper(ctl, scenes):
    """Type 2 through the evaluator, a description without a record, and helpers.camera_rays' formula (float64,
    the same jitter): one ray set."""
    _, d = scenes["perspective"]
    _, d0 = SC.quad_scene(ctl, "perspective", sensor=False)
    assert not d0.sensor and bytes(d0.camera) == bytes(d.camera)
    want = camera_rays(d, SC.W, SC.H, seed=3)
    rng = np.random.default_rng(3)
    ys, xs = np.mgrid[0:SC.H, 0:SC.W]
    pX = np.stack([xs.ravel() + rng.random(SC.W * SC.H), ys.ravel() + rng.random(SC.W * SC.H)], 1)
    q = SC.queries(ctl, pX.astype(np.float32), np.zeros((len(pX), 2), np.float32), True)
    got = ctl.host_sensor_eval(d, q)
    assert got.tobytes() == ctl.host_sensor_eval(d0, q).tobytes()
    # the helper's pixel sample is float64, the query's its fp32 rounding: at most EPS * 48 in x, which moves
    # the direction by less than one more rounding of the chain above
    err_d = np.linalg.norm(got["d"].astype(np.float64) - want[:, 4:7].astype(np.float64), axis=1).max()
    err_o = np.linalg.norm(got["o"].astype(np.float64) - want[:, 0:3].astype(np.float64), axis=1).max()
    print(f"perspective vs helpers.camera_rays: direction {err_d / (K['perspective'] * EPS):.3f}, origin {err_o / (K['perspective'] * EPS * 4.1):.3f} of the tolerance")
    assert err_d <= (K['perspective'] + 2) * EPS and err_o <= K['perspective'] * EPS * 4.1      # want is fp32 itself: one more rounding each


# ---------------------------------------------------------------------------------------------
def _tw(d):
    return np.array(d.camera.to_world.m[:], np.float64).reshape(4, 4)


def _to_camera(d, p):
    tw = _tw(d)
    return (np.asarray(p, np.float64) - tw[:3, 3]) @ tw[:3, :3]          # the rotation is orthonormal (SC.CAM)


def _translation32(d):
    return np.array([d.camera.to_world.m[3], d.camera.to_world.m[7], d.camera.to_world.m[11]], np.float32)


def _forward32(d):
    return np.array([d.camera.to_world.m[2], d.camera.to_world.m[6], d.camera.to_world.m[10]], np.float32)


def _fixed_pixel(ctl, differential, pixel=(13.25, 20.5), n=512, seed=4):
    rng = np.random.default_rng(seed)
    return SC.queries(ctl, np.tile(np.array(pixel, np.float32), (n, 1)), rng.random((n, 2)).astype(np.float32), differential)


@pytest.mark.parametrize("differential", [False, True])
def test_thin_lens_closed_forms(ctl, scenes, differential):
    _, d = scenes["thinlens"]
    f = SC.SENSORS["thinlens"]["focus_distance"]
    q = _fixed_pixel(ctl, differential)
    r = ctl.host_sensor_eval(d, q)
    # every ray of one pixel sample passes through toWorld(focusP): the point at camera-space z = f on the ray
    o, dr = _to_camera(d, r["o"]), r["d"].astype(np.float64) @ _tw(d)[:3, :3]
    focus = o + dr * ((f - o[:, 2]) / dr[:, 2])[:, None]
    spread = np.abs(focus - focus.mean(axis=0)).max()
    lens = np.linalg.norm(o[:, :2], axis=1)
    assert lens.max() > 0.9 * SC.SENSORS["thinlens"]["aperture_radius"] and np.abs(o[:, 2]).max() <= K['thinlens'] * EPS * 4.1
    # the direction's K['thinlens'] EPS over the distance to the focal plane, plus the origin's K['thinlens'] EPS SCALE
    tol = K['thinlens'] * EPS * (np.linalg.norm(focus, axis=1).max() + 4.1 + lens.max())
    print(f"thin lens: focus spread / tolerance {spread / tol:.3f}")
    assert spread <= tol
    # the lens centre is toWorld.Translation() itself
    c = ctl.host_sensor_eval(d, SC.queries(ctl, q["pixel_sample"][:4], np.full((4, 2), 0.5, np.float32), differential))
    assert np.array_equal(c["o"], np.tile(_translation32(d), (4, 1)))


def test_orthographic_closed_forms(ctl, scenes):
    _, d = scenes["orthographic"]
    near = 1.0                                             # set_camera's near plane
    for differential in (False, True):
        q = SC.random_queries(ctl, differential, n=512, seed=6)
        r = ctl.host_sensor_eval(d, q)
        assert np.array_equal(r["d"], np.tile(_forward32(d), (len(q), 1)))           # toWorld.Forward(), bit for bit
        if differential:
            assert np.array_equal(r["dx"], r["d"]) and np.array_equal(r["dy"], r["d"])
        o = _to_camera(d, r["o"])
        # sampleRay starts on the plane z = 0 of camera space, sampleRayDifferential at nearP, z = near
        z = near if differential else 0.0
        assert np.abs(o[:, 2] - z).max() <= K['orthographic'] * EPS * (4.1 + 2.0), np.abs(o[:, 2] - z).max()
        # affine in the pixel sample: a least-squares plane through (x, y) -> o leaves rounding only
        A = np.concatenate([q["pixel_sample"].astype(np.float64), np.ones((len(q), 1))], 1)
        res = r["o"].astype(np.float64) - A @ np.linalg.lstsq(A, r["o"].astype(np.float64), rcond=None)[0]
        assert np.abs(res).max() <= K['orthographic'] * EPS * (4.1 + 2.0), np.abs(res).max()
        # and the view is the one the matrices say: x in [-1, 1], y in [-1 / aspect, 1 / aspect], mirrored
        assert np.abs(o[:, 0]).max() <= 1.0 + 1e-5 and np.abs(o[:, 1]).max() <= SC.H / SC.W + 1e-5


@pytest.mark.parametrize("differential", [False, True])
def test_telecentric_closed_forms(ctl, scenes, differential):
    _, d = scenes["telecentric"]
    S = SC.SENSORS["telecentric"]
    q = _fixed_pixel(ctl, differential)
    r = ctl.host_sensor_eval(d, q)
    o, dr = _to_camera(d, r["o"]), r["d"].astype(np.float64) @ _tw(d)[:3, :3]
    meet = o + dr * ((S["focus_distance"] - o[:, 2]) / dr[:, 2])[:, None]
    spread = np.abs(meet - meet.mean(axis=0)).max()
    tol = K['telecentric'] * EPS * (np.linalg.norm(meet, axis=1).max() + 4.1 + 1.0)
    print(f"telecentric: focus spread / tolerance {spread / tol:.3f}")
    assert spread <= tol
    lens = np.linalg.norm(o[:, :2] - meet[:, :2], axis=1)
    assert lens.max() > 0.9 * S["aperture_radius"] / S["screen_scale"][0] and lens.max() <= S["aperture_radius"] / S["screen_scale"][0] + 1e-6
    c = ctl.host_sensor_eval(d, SC.queries(ctl, q["pixel_sample"][:4], np.full((4, 2), 0.5, np.float32), differential))
    assert np.linalg.norm(c["d"].astype(np.float64) - _forward32(d).astype(np.float64), axis=1).max() <= K['telecentric'] * EPS


def test_spherical_closed_forms(ctl, scenes):
    _, d = scenes["spherical"]
    centre = ctl.host_sensor_eval(d, SC.queries(ctl, [(SC.W / 2.0, SC.H / 2.0)], [(0.3, 0.7)], False))
    assert np.linalg.norm(centre["d"][0].astype(np.float64) - _forward32(d).astype(np.float64)) <= K['spherical'] * EPS
    for differential in (False, True):
        q = SC.random_queries(ctl, differential, n=1024, seed=8)
        r = ctl.host_sensor_eval(d, q)
        assert np.abs(np.linalg.norm(r["d"].astype(np.float64), axis=1) - 1.0).max() <= K['spherical'] * EPS
        assert np.array_equal(r["o"], np.tile(_translation32(d), (len(q), 1)))
        assert not r["has_differentials"].any() and not r["ox"].any() and not r["dx"].any() and not r["dy"].any()
    # x runs against phi (the 1 - x of the formula): d = (sin phi sin theta, cos theta, -cos phi sin theta) in camera
    # space, so along the image's middle row phi = atan2(d.x, -d.z) in [0, 2 pi) falls as x grows, by 2 pi / w a pixel
    xs = np.linspace(2.0, SC.W - 2.0, 23).astype(np.float32)
    row = ctl.host_sensor_eval(d, SC.queries(ctl, np.stack([xs, np.full_like(xs, SC.H / 2.0)], 1), np.zeros((23, 2)), False))
    dc = row["d"].astype(np.float64) @ _tw(d)[:3, :3]
    phi = np.mod(np.arctan2(dc[:, 0], -dc[:, 2]), 2 * np.pi)
    assert np.allclose(np.diff(phi), -2 * np.pi / SC.W * np.diff(xs.astype(np.float64)), atol=1e-5), phi
    # and y against theta: the top row looks up
    top = ctl.host_sensor_eval(d, SC.queries(ctl, [(10.0, 0.5)], [(0, 0)], False))["d"][0].astype(np.float64) @ _tw(d)[:3, :3]
    assert top[1] < -0.99 or top[1] > 0.99


# ---------------------------------------------------------------------------------------------
BAD_FIELDS = [
    ("type", dict(type=0), "type"), ("type", dict(type=6), "type"),
    ("aperture_radius", dict(type=3, aperture_radius=-0.1, focus_distance=1.0), "aperture_radius"),
    ("aperture_radius", dict(type=3, aperture_radius=float("nan"), focus_distance=1.0), "aperture_radius"),
    ("aperture_radius", dict(type=4, aperture_radius=float("inf")), "aperture_radius"),
    ("focus_distance", dict(type=3, aperture_radius=0.1, focus_distance=0.0), "focus_distance"),
    ("focus_distance", dict(type=5, aperture_radius=0.1, focus_distance=float("nan")), "focus_distance"),
    ("focus_distance", dict(type=5, aperture_radius=0.1, focus_distance=-2.0), "focus_distance"),
    ("screen_scale", dict(type=5, aperture_radius=0.1, focus_distance=1.0, screen_scale=(0.0, 1.0)), "screen_scale"),
    ("screen_scale", dict(type=5, aperture_radius=0.1, focus_distance=1.0, screen_scale=(1.0, float("inf"))), "screen_scale"),
]


def bad_record(ctl, fields):
    r = ctl._abi.Sensor(2, 0.0, 0.0, (C.c_float * 2)(1.0, 1.0))
    for k, v in fields.items():
        setattr(r, k, (C.c_float * 2)(*v) if k == "screen_scale" else v)
    return r


@pytest.mark.parametrize("field,fields,match", BAD_FIELDS)
def test_refusals(ctl, field, fields, match):
    L = ctl.lib()
    s, d = SC.quad_scene(ctl, "thinlens")
    before = bytes(d.sensor[0])
    f = dict(dict(aperture_radius=0.0, focus_distance=0.0, screen_scale=(1.0, 1.0)), **fields)
    status = L.ctl_host_scene_set_sensor(s._h, f["type"], f["aperture_radius"], f["focus_distance"],
                                         (C.c_float * 2)(*f["screen_scale"]))
    assert status != 0 and match in L.ctl_host_last_error().decode()
    d = s.compile()
    assert bytes(d.sensor[0]) == before                                # the scene keeps the sensor it had
    rec = bad_record(ctl, fields)
    d.sensor = C.pointer(rec)
    with pytest.raises(ctl.CTLError, match=match):
        ctl.host_sensor_eval(d, SC.edge_queries(ctl, True))


def test_set_sensor_needs_a_camera_and_a_known_kind(ctl):
    s = ctl.HostScene()
    with pytest.raises(ctl.CTLError, match="set_camera"):
        s.set_sensor("orthographic")
    with pytest.raises(ValueError, match="kind"):
        s.set_sensor("fisheye")
    # fields a type does not read are not checked for it
    _, d = SC.quad_scene(ctl, "orthographic", focus_distance=0.0)
    assert d.sensor[0].type == 4
    _, d = SC.quad_scene(ctl, "spherical", focus_distance=-1.0)
    assert d.sensor[0].type == 1


def test_set_sensor_after_the_compile_refreshes_the_description(ctl):
    """A compiled scene's description takes the new camera and sensor records at once, equal to a fresh compile's."""
    s, d = SC.quad_scene(ctl, "perspective", sensor=False)
    persp = bytes(d.camera)
    s.set_sensor("orthographic")
    assert d.sensor and d.sensor[0].type == 4 and bytes(d.camera) != persp
    _, fresh = SC.quad_scene(ctl, "orthographic")
    assert bytes(d.camera) == bytes(fresh.camera) and bytes(d.sensor[0]) == bytes(fresh.sensor[0])
    s.set_sensor("thinlens", aperture_radius=0.2, focus_distance=3.0)
    assert bytes(d.camera) == persp and d.sensor[0].focus_distance == 3.0     # thin lens computes as perspective does


def test_scene_cache_round_trip(ctl, tmp_path):
    from cudatracerlib_amd import scene_cache
    _, d = SC.quad_scene(ctl, "telecentric")
    path = str(tmp_path / "scene.bin")
    scene_cache.save(d, path)
    c = scene_cache.load(path)
    try:
        assert bytes(c.desc.sensor[0]) == bytes(d.sensor[0])
        q = SC.random_queries(ctl, True, n=64)
        assert ctl.host_sensor_eval(c.desc, q).tobytes() == ctl.host_sensor_eval(d, q).tobytes()
    finally:
        c.close()
    _, d0 = SC.quad_scene(ctl, "perspective", sensor=False)
    scene_cache.save(d0, path)
    c = scene_cache.load(path)
    try:
        assert not c.desc.sensor
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------
ABI_PROBE = r"""
#include "ctl_trace.h"
#include <stdio.h>
#include <stddef.h>
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu\n", sizeof(ctl_sensor), sizeof(ctl_sensor_query), sizeof(ctl_sensor_result),
           offsetof(ctl_scene_desc, sensor), offsetof(ctl_scene_desc, materials_ext), sizeof(ctl_scene_desc));
    return 0;
}
"""


def test_abi(ctl, tmp_path):
    A = ctl._abi
    L = ctl.lib()
    for name in ("ctl_sensor_eval", "ctl_host_sensor_eval", "ctl_host_scene_set_sensor", "ctl_host_scene_sensor_state"):
        assert getattr(L, name) is not None
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    assert cc is not None, "no host C compiler"
    src, exe = tmp_path / "abi_probe.c", tmp_path / "abi_probe"
    src.write_text(ABI_PROBE)
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    sizes = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert sizes == [C.sizeof(A.Sensor), C.sizeof(A.SensorQuery), C.sizeof(A.SensorResult), A.SceneDesc.sensor.offset,
                     A.SceneDesc.materials_ext.offset, C.sizeof(A.SceneDesc)]
    assert sizes[:3] == [32, 20, 80] and sizes[4] == sizes[3] + 8 and sizes[5] == sizes[4] + 8
    assert ctl.SENSOR_QUERY_DTYPE.itemsize == 20 and ctl.SENSOR_RESULT_DTYPE.itemsize == 80
    assert A.SceneDesc.sensor.offset == A.SceneDesc.volumes.offset + 16


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator", ["pt", "wpt", "prim"])
@pytest.mark.parametrize("kind", SC.NEW_KINDS)
def test_the_quad_replay_meets_its_conditions(ctl, scenes, kind, integrator):
    """The float64 replay that test_gpu_sensors.py holds the renders to, alone: at most 2 % of the paths left
    out, at least 1 / 8 of the pixels seeing the quad and 1 / 8 missing it, under every sensor and integrator;
    and for the two lens sensors the aperture matters (the quad is off the focus distance)."""
    _, d = scenes[kind]
    rp = SC.replay(ctl, d, integrator, SC.host_draws(ctl, 0))
    n = SC.W * SC.H
    assert len(rp["pixel"]) == n
    ok = ~rp["skip"]
    print(f"{kind} {integrator}: hit {int((rp['hit'] & ok).sum())}, miss {int((~rp['hit'] & ok).sum())}, left out {int(rp['skip'].sum())}")
    assert rp["skip"].sum() <= 0.02 * n
    assert (rp["hit"] & ok).sum() >= n // 8 and (~rp["hit"] & ok).sum() >= n // 8
    if kind in ("thinlens", "telecentric"):
        q0 = rp["q"].copy()
        q0["aperture_sample"] = 0.5
        hit0, _ = SC.quad_hit(*[ctl.host_sensor_eval(d, q0)[f] for f in ("o", "d")])
        assert (hit0 != rp["hit"]).sum() >= 4, "the aperture sample decides no pixel"


def test_the_near_quad_tells_the_orthographic_origins_apart(ctl):
    """The quad at camera-space z = 0.5, in front of sampleRay's origins (z = 0) and behind
    sampleRayDifferential's (nearP, z = near = 1): the WavefrontPathTracer's replay sees the quad in at least 1 / 8
    of the pixels and misses it in 1 / 8, the PathTracer's and the PrimTracer's see it nowhere.  The direction is
    toWorld.Forward() = +z exactly, so which side of the quad an origin lies on rests on no rounding."""
    _, d = SC.near_quad_scene(ctl)
    n = SC.W * SC.H
    draws = SC.host_draws(ctl, 0)
    rp = SC.replay(ctl, d, "wpt", draws, quad_z=SC.NEAR_QUAD_Z)
    assert np.array_equal(rp["rays"]["d"], np.tile(np.array([0, 0, 1], np.float32), (n, 1)))
    assert np.all(rp["rays"]["o"][:, 2] == np.float32(-4.0))
    ok = ~rp["skip"]
    assert rp["skip"].sum() <= 0.02 * n and (rp["hit"] & ok).sum() >= n // 8 and (~rp["hit"] & ok).sum() >= n // 8
    for integrator in ("pt", "prim"):
        rp = SC.replay(ctl, d, integrator, draws, quad_z=SC.NEAR_QUAD_Z)
        assert np.all(rp["rays"]["o"][:, 2] == np.float32(-3.0))
        assert not rp["hit"].any() and not rp["skip"].any()
