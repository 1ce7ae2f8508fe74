"""Light::sampleDirect of the point, spot and distant lights in float64 numpy, written from the
formulas (SceneTypes/Light.cu:16-31, 223-244, 287-302, 327-336), not from csrc/ctl_light.h: no
frame, no fp32 intermediate, no shared code.  Every function takes (n, 3) reference points and
returns a dict of float64 arrays; inputs are the fp32-representable numbers the scene was built from.

A delta light is a Dirac in position (point, spot) or direction (distant): the sample is the one
point, pdf 1 in the discrete measure, and the returned value is the irradiance arriving along -d
per unit area normal to d: I / dist^2, I * falloff / dist^2, or the distant light's E."""
import numpy as np

DISCRETE = 4   # EMeasure::EDiscrete


def _f64(a):
    return np.asarray(a, np.float64)


def _towards(pos, ref):
    pos, ref = _f64(pos), _f64(ref).reshape(-1, 3)
    v = pos[None, :] - ref
    dist = np.linalg.norm(v, axis=1)
    return v / dist[:, None], dist


def point(pos, intensity, ref):
    d, dist = _towards(pos, ref)
    return {"value": _f64(intensity)[None, :] / (dist * dist)[:, None], "d": d, "dist": dist,
            "p": np.broadcast_to(_f64(pos), d.shape), "n": np.zeros_like(d), "pdf": np.ones_like(dist)}


def falloff(cos_theta, cutoff_deg, beam_deg):
    """SpotLight::falloffCurve: 0 at and outside the cutoff angle, 1 at and inside the beam width,
    linear in the angle between them."""
    cutoff, beam = np.radians(np.float64(cutoff_deg)), np.radians(np.float64(beam_deg))
    theta = np.arccos(np.clip(cos_theta, -1.0, 1.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        ramp = (cutoff - theta) / (cutoff - beam)
    return np.where(cos_theta <= np.cos(cutoff), 0.0, np.where(cos_theta >= np.cos(beam), 1.0, ramp))


def spot_cos_theta(pos, target, ref):
    """Cosine of the angle between the spot's axis and the direction from the light to ref."""
    d, _ = _towards(pos, ref)
    axis = _f64(target) - _f64(pos)
    axis = axis / np.linalg.norm(axis)
    return -(d @ axis)


def spot(pos, target, intensity, cutoff_deg, beam_deg, ref):
    r = point(pos, intensity, ref)
    r["cos_theta"] = spot_cos_theta(pos, target, ref)
    r["falloff"] = falloff(r["cos_theta"], cutoff_deg, beam_deg)
    r["unattenuated"] = r["value"]
    r["value"] = r["value"] * r["falloff"][:, None]
    return r


def distant(irradiance, direction, scene_radius, ref):
    """The light travels along direction (d, the sample's direction, is -direction).  Its emitting
    disk has radius 1.1 * scene_radius and is centred at direction * radius about the origin; a
    reference point behind the disk's plane (ref . direction < radius) gets nothing (value 0, pdf 0,
    the rest undefined).  1.1 is the reference's float literal 1.1f."""
    ref = _f64(ref).reshape(-1, 3)
    dn = _f64(direction) / np.linalg.norm(_f64(direction))
    radius = np.float64(scene_radius) * np.float64(np.float32(1.1))
    distance = ref @ dn - radius
    lit = distance >= 0
    n = np.broadcast_to(dn, ref.shape)
    return {"value": np.where(lit[:, None], _f64(irradiance)[None, :], 0.0), "d": -n, "dist": distance,
            "p": ref - distance[:, None] * dn[None, :], "n": n, "pdf": lit.astype(np.float64), "distance": distance,
            "radius": radius, "lit": lit}
