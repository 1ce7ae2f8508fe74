// ctl_sensor.h — the five sensors of the reference's Sensor aggregate (SceneTypes/Sensor.h:527),
// fp32 in the reference's operation order, compiled for gfx950 and for the host: one statement of
// Sensor::sampleRay and of Sensor::sampleRayDifferential, which the kernels (device/shading.h), the
// batch evaluators (device/sensor_eval.hip) and the host scene compiler all call.
//
//   sensor_sample_ray               SphericalSensor    Sensor.cu:6-16
//   sensor_sample_ray_differential  PerspectiveSensor  Sensor.cu:102-144
//                                   ThinLensSensor     Sensor.cu:267-311
//                                   OrthographicSensor Sensor.cu:429-450
//                                   TelecentricSensor  Sensor.cu:537-573
//   sensor_update                   the types' Update() (Sensor.cu:76-96, 226-246, 408-427, 515-535):
//                                   m_sampleToCamera, m_dx, m_dy
//   sensor_check                    what upload, update and the host compiler refuse
//
// The PathTracer and the PrimTracer call sampleRayDifferential (PathTracer.cu:190, PrimTracer.cu:22),
// the WavefrontPathTracer sampleRay (WavefrontPathTracer.cu:38).  The two differ in more than rayX
// and rayY: the orthographic sampleRay starts at (nearP.x, nearP.y, 0), its sampleRayDifferential at
// nearP with its own z.
// One departure: SphericalSensor::sampleRayDifferential is its sampleRay and writes
// neither rayX nor rayY, so the reference's computePartials reads uninitialised rays; here the
// function reports that there are none and the path carries no UV partials.
#pragma once
#include "ctl_shade.h"

namespace ctl {

// the record of a description without one: the PerspectiveSensor
CTL_HD ctl_sensor sensor_default() {
    ctl_sensor R;
    R.type = CTL_SENSOR_PERSPECTIVE;
    R.aperture_radius = 0.0f; R.focus_distance = 0.0f;
    R.screen_scale[0] = R.screen_scale[1] = 1.0f;
    R.pad[0] = R.pad[1] = R.pad[2] = 0;
    return R;
}

CTL_HD bool sensor_finite(float x) { return x - x == 0.0f; }

// null, or why the record is refused (the message names the field)
CTL_HD const char* sensor_check(const ctl_sensor& R) {
    if (R.type < CTL_SENSOR_SPHERICAL || R.type > CTL_SENSOR_TELECENTRIC) return "sensor type is not one of 1-5";
    if (!sensor_finite(R.aperture_radius) || R.aperture_radius < 0.0f)
        return "sensor aperture_radius must be finite and not negative";
    const bool lens = R.type == CTL_SENSOR_THINLENS || R.type == CTL_SENSOR_TELECENTRIC;
    if (lens && (!sensor_finite(R.focus_distance) || !(R.focus_distance > 0.0f)))
        return "sensor focus_distance must be finite and positive";
    if (R.type == CTL_SENSOR_TELECENTRIC &&
        (!sensor_finite(R.screen_scale[0]) || !sensor_finite(R.screen_scale[1]) || !(R.screen_scale[0] > 0.0f) ||
         !(R.screen_scale[1] > 0.0f)))
        return "sensor screen_scale must be finite and positive";
    return nullptr;
}

CTL_HD bool sensor_is_orthographic(uint32_t type) {
    return type == CTL_SENSOR_ORTHOGRAPHIC || type == CTL_SENSOR_TELECENTRIC;
}

// m_sampleToCamera.TransformPoint(pixelSample * m_invResolution, 0): nearP (focusP before its z is set)
CTL_HD f3 sensor_near_point(const ctl_camera& C, f2 pX) {
    return xform_point(to_m44(C.sample_to_camera), mk3(pX.x * C.inv_resolution[0], pX.y * C.inv_resolution[1], 0.0f));
}

// the lens point of the thin-lens (scale = m_apertureRadius) and telecentric (m_apertureRadius / screenScale.x) sensors
CTL_HD f2 sensor_lens_point(f2 apertureSample, float scale) {
    return square_to_uniform_disk_concentric(apertureSample) * scale;
}

CTL_HD f3 sensor_spherical_dir(const ctl_camera& C, f2 pX) {
    const float phi = (1.0f - pX.x * C.inv_resolution[0]) * 2 * CTL_PI;
    const float theta = (1.0f - pX.y * C.inv_resolution[1]) * CTL_PI;
    const float sinPhi = cr_sin(phi), cosPhi = cr_cos(phi), sinTheta = cr_sin(theta), cosTheta = cr_cos(theta);
    return mk3(sinPhi * sinTheta, cosTheta, -cosPhi * sinTheta);
}

// Sensor::sampleRay
CTL_HD void sensor_sample_ray(const ctl_camera& C, const ctl_sensor& R, f2 pX, f2 ap, f3& o, f3& d) {
    const m44 tw = to_m44(C.to_world);
    switch (R.type) {
    case CTL_SENSOR_SPHERICAL:
        o = xform_point(tw, mk3s(0.0f));
        d = xform_dir(tw, sensor_spherical_dir(C, pX));
        break;
    case CTL_SENSOR_THINLENS: {
        const f2 tmp = sensor_lens_point(ap, R.aperture_radius);
        const f3 nearP = sensor_near_point(C, pX);
        const f3 apertureP = mk3(tmp.x, tmp.y, 0.0f);
        const f3 focusP = nearP * (R.focus_distance / nearP.z);
        o = xform_point(tw, apertureP);
        d = xform_dir(tw, normalize(focusP - apertureP));
        break;
    }
    case CTL_SENSOR_ORTHOGRAPHIC: {
        const f3 nearP = sensor_near_point(C, pX);
        o = xform_point(tw, mk3(nearP.x, nearP.y, 0.0f));
        d = xform_dir(tw, mk3(0.0f, 0.0f, 1.0f));
        break;
    }
    case CTL_SENSOR_TELECENTRIC: {
        const f2 disk = sensor_lens_point(ap, R.aperture_radius / R.screen_scale[0]);
        f3 focusP = sensor_near_point(C, pX);
        focusP.z = R.focus_distance;
        const f3 orig = mk3(disk.x + focusP.x, disk.y + focusP.y, 0.0f);
        o = xform_point(tw, orig);
        d = normalize(xform_dir(tw, focusP - orig));
        break;
    }
    default:   // CTL_SENSOR_PERSPECTIVE
        o = xform_point(tw, mk3s(0.0f));
        d = xform_dir(tw, normalize(sensor_near_point(C, pX)));
        break;
    }
}

// Sensor::sampleRayDifferential; false: rayX and rayY are not defined (and are left unwritten)
CTL_HD bool sensor_sample_ray_differential(const ctl_camera& C, const ctl_sensor& R, f2 pX, f2 ap, f3& o, f3& d,
                                           f3& oX, f3& dX, f3& oY, f3& dY) {
    const m44 tw = to_m44(C.to_world);
    const f3 mdx = mk3(C.dx[0], C.dx[1], C.dx[2]), mdy = mk3(C.dy[0], C.dy[1], C.dy[2]);
    switch (R.type) {
    case CTL_SENSOR_SPHERICAL:
        sensor_sample_ray(C, R, pX, ap, o, d);
        return false;
    case CTL_SENSOR_THINLENS: {
        const f2 tmp = sensor_lens_point(ap, R.aperture_radius);
        const f3 nearP = sensor_near_point(C, pX);
        const f3 apertureP = mk3(tmp.x, tmp.y, 0.0f);
        const float fDist = R.focus_distance / nearP.z;
        const f3 focusP = nearP * fDist, focusPx = (nearP + mdx) * fDist, focusPy = (nearP + mdy) * fDist;
        o = xform_point(tw, apertureP);
        d = xform_dir(tw, normalize(focusP - apertureP));
        oX = oY = o;
        dX = xform_dir(tw, normalize(focusPx - apertureP));
        dY = xform_dir(tw, normalize(focusPy - apertureP));
        return true;
    }
    case CTL_SENSOR_ORTHOGRAPHIC: {
        const f3 nearP = sensor_near_point(C, pX);
        o = xform_point(tw, nearP);
        d = xform_dir(tw, mk3(0.0f, 0.0f, 1.0f));
        oX = xform_point(tw, nearP + mdx);
        oY = xform_point(tw, nearP + mdy);
        dX = dY = d;
        return true;
    }
    case CTL_SENSOR_TELECENTRIC: {
        const f2 disk = sensor_lens_point(ap, R.aperture_radius / R.screen_scale[0]);
        f3 focusP = sensor_near_point(C, pX);
        focusP.z = R.focus_distance;
        const f3 orig = mk3(disk.x + focusP.x, disk.y + focusP.y, 0.0f);
        o = xform_point(tw, orig);
        d = normalize(xform_dir(tw, focusP - orig));
        oX = xform_point(tw, orig + mdx);
        oY = xform_point(tw, orig + mdy);
        dX = dY = d;
        return true;
    }
    default: {   // CTL_SENSOR_PERSPECTIVE
        const f3 nearP = sensor_near_point(C, pX);
        o = xform_point(tw, mk3s(0.0f));
        d = xform_dir(tw, normalize(nearP));
        oX = oY = o;
        dX = xform_dir(tw, normalize(nearP + mdx));
        dY = xform_dir(tw, normalize(nearP + mdy));
        return true;
    }
    }
}

// The types' Update(): m_cameraToSample = Scale(-0.5, -0.5 aspect, 1) % Translate(-1, -1 / aspect, 0) % proj with
// proj = float4x4::Perspective(fov, near, far) (spherical, perspective, thin lens: SensorBase's and their own) or
// float4x4::orthographic(near, far) = Scale(1, 1, 1 / (far - near)) % Translate(0, 0, -near) (orthographic,
// telecentric); m_sampleToCamera its inverse; m_dx, m_dy the steps of one pixel.  fov in radians.
CTL_HD void sensor_update(uint32_t type, float fov, float nearc, float farc, float resx, float resy, m44& s2c, f3& dx,
                          f3& dy) {
    const float invx = 1.0f / resx, invy = 1.0f / resy;   // Vec2f(1) / m_resolution
    const float aspect = resx / resy;
    m44 sc = m44_identity(); sc.at(0, 0) = -0.5f; sc.at(1, 1) = -0.5f * aspect; sc.at(2, 2) = 1.0f;
    m44 tl = m44_identity(); tl.at(0, 3) = -1.0f; tl.at(1, 3) = -1.0f / aspect; tl.at(2, 3) = 0.0f;
    m44 proj;
    if (sensor_is_orthographic(type)) {
        m44 s = m44_identity(); s.at(2, 2) = 1.0f / (farc - nearc);
        m44 t = m44_identity(); t.at(2, 3) = -nearc;
        proj = matmul(s, t);
    } else {
        const float recip = 1.0f / (farc - nearc);            // float4x4::Perspective
        const float cot = 1.0f / cr_tan(fov / 2.0f);
        proj = m44_zero();
        proj.at(0, 0) = cot; proj.at(1, 1) = cot; proj.at(2, 2) = farc * recip; proj.at(2, 3) = -nearc * farc * recip;
        proj.at(3, 2) = 1;
    }
    s2c = inverse(matmul(matmul(sc, tl), proj));
    dx = xform_point(s2c, mk3(invx, 0.0f, 0.0f)) - xform_point(s2c, mk3s(0.0f));
    dy = xform_point(s2c, mk3(0.0f, invy, 0.0f)) - xform_point(s2c, mk3s(0.0f));
}

}  // namespace ctl
