"""Float64 statement of Sensor::sampleRay and Sensor::sampleRayDifferential for the reference's five
sensor types (spherical 1, perspective 2, thin lens 3, orthographic 4, telecentric 5), written from the
formulas of SceneTypes/Sensor.cu, not from the library's code: ten functions, vectorised over queries.

A camera is a dict of float64 arrays taken from the fp32 ctl_camera record (tw, s2c 4x4; dx, dy 3; inv 2), a
sensor a dict (type, aperture_radius, focus_distance, screen_scale).  PI is the reference's fp32 constant."""
import numpy as np

SPHERICAL, PERSPECTIVE, THINLENS, ORTHOGRAPHIC, TELECENTRIC = 1, 2, 3, 4, 5
KINDS = {"spherical": 1, "perspective": 2, "thinlens": 3, "orthographic": 4, "telecentric": 5}
PI = np.float64(np.float32(3.14159265358979))


def camera(desc):
    c = desc.camera
    return dict(tw=np.array(c.to_world.m[:], np.float64).reshape(4, 4),
                s2c=np.array(c.sample_to_camera.m[:], np.float64).reshape(4, 4),
                dx=np.array(c.dx[:], np.float64), dy=np.array(c.dy[:], np.float64),
                inv=np.array(c.inv_resolution[:], np.float64), width=c.width, height=c.height)


def sensor(desc):
    if not desc.sensor:
        return dict(type=PERSPECTIVE, aperture_radius=0.0, focus_distance=0.0, screen_scale=(1.0, 1.0))
    r = desc.sensor[0]
    return dict(type=int(r.type), aperture_radius=np.float64(r.aperture_radius), focus_distance=np.float64(r.focus_distance),
                screen_scale=(np.float64(r.screen_scale[0]), np.float64(r.screen_scale[1])))


def point(M, p):
    """float4x4::TransformPoint: the homogeneous product divided by w"""
    q = np.concatenate([p, np.ones((p.shape[0], 1))], 1) @ M.T
    return q[:, :3] / q[:, 3:4]


def direction(M, d):
    return d @ M[:3, :3].T


def unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def disk(ap):
    """Warp::squareToUniformDiskConcentric"""
    r1, r2 = 2.0 * ap[:, 0] - 1.0, 2.0 * ap[:, 1] - 1.0
    zero = (r1 == 0) & (r2 == 0)
    first = ~zero & (r1 * r1 > r2 * r2)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(zero, 0.0, np.where(first, r1, r2))
        phi = np.where(zero, 0.0, np.where(first, (PI / 4.0) * (r2 / r1), (PI / 2.0) - (r1 / r2) * (PI / 4.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi)], 1)


def near_point(cam, pX):
    n = pX.shape[0]
    return point(cam["s2c"], np.stack([pX[:, 0] * cam["inv"][0], pX[:, 1] * cam["inv"][1], np.zeros(n)], 1))


def _z0(xy):
    return np.concatenate([xy, np.zeros((xy.shape[0], 1))], 1)


def _forward(cam, n):
    return np.broadcast_to(direction(cam["tw"], np.array([[0.0, 0.0, 1.0]])), (n, 3)).copy()


# ---- sampleRay ----------------------------------------------------------------------------------
def spherical_ray(cam, S, pX, ap):
    phi = (1.0 - pX[:, 0] * cam["inv"][0]) * 2 * PI
    theta = (1.0 - pX[:, 1] * cam["inv"][1]) * PI
    d = np.stack([np.sin(phi) * np.sin(theta), np.cos(theta), -np.cos(phi) * np.sin(theta)], 1)
    o = np.broadcast_to(point(cam["tw"], np.zeros((1, 3))), d.shape).copy()
    return o, direction(cam["tw"], d)


def perspective_ray(cam, S, pX, ap):
    d = unit(near_point(cam, pX))
    o = np.broadcast_to(point(cam["tw"], np.zeros((1, 3))), d.shape).copy()
    return o, direction(cam["tw"], d)


def thinlens_ray(cam, S, pX, ap):
    aperture = _z0(disk(ap) * S["aperture_radius"])
    nearP = near_point(cam, pX)
    focusP = nearP * (S["focus_distance"] / nearP[:, 2:3])
    return point(cam["tw"], aperture), direction(cam["tw"], unit(focusP - aperture))


def orthographic_ray(cam, S, pX, ap):
    nearP = near_point(cam, pX)
    return point(cam["tw"], _z0(nearP[:, :2])), _forward(cam, pX.shape[0])


def _telecentric_points(cam, S, pX, ap):
    d = disk(ap) * (S["aperture_radius"] / S["screen_scale"][0])
    focusP = near_point(cam, pX)
    focusP[:, 2] = S["focus_distance"]
    return focusP, _z0(d + focusP[:, :2])


def telecentric_ray(cam, S, pX, ap):
    focusP, orig = _telecentric_points(cam, S, pX, ap)
    return point(cam["tw"], orig), unit(direction(cam["tw"], focusP - orig))


# ---- sampleRayDifferential: (o, d, oX, dX, oY, dY), or None for rayX / rayY where undefined ----------
def spherical_ray_differential(cam, S, pX, ap):
    o, d = spherical_ray(cam, S, pX, ap)          # rayX and rayY are never written
    return o, d, None, None, None, None


def perspective_ray_differential(cam, S, pX, ap):
    nearP = near_point(cam, pX)
    o, d = perspective_ray(cam, S, pX, ap)
    return (o, d, o, direction(cam["tw"], unit(nearP + cam["dx"])), o, direction(cam["tw"], unit(nearP + cam["dy"])))


def thinlens_ray_differential(cam, S, pX, ap):
    aperture = _z0(disk(ap) * S["aperture_radius"])
    nearP = near_point(cam, pX)
    fDist = S["focus_distance"] / nearP[:, 2:3]
    o = point(cam["tw"], aperture)
    f = lambda q: direction(cam["tw"], unit(q * fDist - aperture))
    return o, f(nearP), o, f(nearP + cam["dx"]), o, f(nearP + cam["dy"])


def orthographic_ray_differential(cam, S, pX, ap):
    nearP = near_point(cam, pX)
    d = _forward(cam, pX.shape[0])
    return point(cam["tw"], nearP), d, point(cam["tw"], nearP + cam["dx"]), d, point(cam["tw"], nearP + cam["dy"]), d


def telecentric_ray_differential(cam, S, pX, ap):
    focusP, orig = _telecentric_points(cam, S, pX, ap)
    d = unit(direction(cam["tw"], focusP - orig))
    return point(cam["tw"], orig), d, point(cam["tw"], orig + cam["dx"]), d, point(cam["tw"], orig + cam["dy"]), d


RAY = {SPHERICAL: spherical_ray, PERSPECTIVE: perspective_ray, THINLENS: thinlens_ray, ORTHOGRAPHIC: orthographic_ray,
       TELECENTRIC: telecentric_ray}
RAY_DIFFERENTIAL = {SPHERICAL: spherical_ray_differential, PERSPECTIVE: perspective_ray_differential,
                    THINLENS: thinlens_ray_differential, ORTHOGRAPHIC: orthographic_ray_differential,
                    TELECENTRIC: telecentric_ray_differential}


def sample_ray(cam, S, pX, ap):
    return RAY[S["type"]](cam, S, np.asarray(pX, np.float64), np.asarray(ap, np.float64))


def sample_ray_differential(cam, S, pX, ap):
    return RAY_DIFFERENTIAL[S["type"]](cam, S, np.asarray(pX, np.float64), np.asarray(ap, np.float64))
