// ctl_light.h — the delta lights (PointLight, SpotLight, DistantLight,
// SceneTypes/Light.h:34-94, 145-292) for the host scene compiler and the device
// kernels, fp32 in the reference's operation order, and the Light::sampleDirect
// dispatch over all five kinds of ctl_light.  A delta light is never hit: eval
// is 0 and pdfDirect is 1 in the discrete measure, so it enters only through the
// light sample of the integrators.
//
//   point_sample_direct     PointLight::sampleDirect    SceneTypes/Light.cu:16-31
//   distant_sample_direct   DistantLight::sampleDirect  SceneTypes/Light.cu:223-244
//   spot_sample_direct      SpotLight::sampleDirect     SceneTypes/Light.cu:287-302
//   spot_falloff            SpotLight::falloffCurve     SceneTypes/Light.cu:327-336
//   delta_pdf_direct        pdfDirect of the three      SceneTypes/Light.h:61-64
//   spot_params / distant_params  the constructors and Update() (Light.cu:268-277, Light.h:159-173)
//   light_sample_direct_any Light::sampleDirect over the aggregate
#pragma once
#include "ctl_env.h"

namespace ctl {

static_assert(sizeof(ctl_light_params) == sizeof(ctl_light_tri), "a delta light's parameters fill one light_tris slot");

CTL_HD float radians_ref(float deg) { return (CTL_PI / 180.f) * deg; }   // math::Radians (MathFunc.h:182-185)

// The slot of a delta light: light_tris[L.tri_first] read as ctl_light_params (include/ctl_trace.h).
CTL_HD const ctl_light_params& light_params(const ctl_light& L, const ctl_light_tri* tris) {
    return *reinterpret_cast<const ctl_light_params*>(tris + L.tri_first);
}
CTL_HD frame params_frame(const ctl_light_params& P) {
    frame f;
    f.s = mk3(P.s[0], P.s[1], P.s[2]); f.t = mk3(P.t[0], P.t[1], P.t[2]); f.n = mk3(P.n[0], P.n[1], P.n[2]);
    return f;
}
CTL_HD void params_set_frame(ctl_light_params& P, f3 n) {   // Frame(n)
    f3 s, t;
    coordinate_system(n, s, t);
    P.s[0] = s.x; P.s[1] = s.y; P.s[2] = s.z;
    P.t[0] = t.x; P.t[1] = t.y; P.t[2] = t.z;
    P.n[0] = n.x; P.n[1] = n.y; P.n[2] = n.z;
}

// SpotLight(p, t, L, width, fall): width is the cutoff angle, fall the beam width, in degrees
CTL_HD ctl_light_params spot_params(f3 pos, f3 target, float cutoff_deg, float beam_deg) {
    ctl_light_params P{};
    P.pos[0] = pos.x; P.pos[1] = pos.y; P.pos[2] = pos.z;
    params_set_frame(P, normalize(target - pos));
    const float cutoff = radians_ref(cutoff_deg), beam = radians_ref(beam_deg);
    P.cos_beam_width = cr_cos(beam);
    P.cos_cutoff_angle = cr_cos(cutoff);
    P.cutoff_angle = cutoff;
    P.inv_transition_width = 1.0f / (cutoff - beam);
    return P;
}
// DistantLight(L, d, r): d normalised by the caller as the constructor's NormalizedT argument
CTL_HD ctl_light_params distant_params(f3 d, float scene_radius) {
    ctl_light_params P{};
    params_set_frame(P, d);
    P.cos_beam_width = scene_radius * 1.1f;   // radius
    return P;
}

CTL_HD spec light_intensity(const ctl_light& L) { return mk3(L.radiance[0], L.radiance[1], L.radiance[2]); }

// The part PointLight and SpotLight share: dRec towards `pos`; returns invDist
CTL_HD float delta_position_rec(f3 pos, direct_rec& dRec) {
    dRec.p = pos;
    const f3 dir = dRec.p - dRec.ref;
    dRec.dist = length(dir);
    const float invDist = 1.0f / dRec.dist;
    dRec.d = dir * invDist;
    dRec.n = mk3s(0.0f);
    dRec.pdf = 1;
    dRec.measure = kEDiscrete;
    return invDist;
}

CTL_HD spec point_sample_direct(const ctl_light& L, const ctl_light_params& P, direct_rec& dRec) {
    const float invDist = delta_position_rec(mk3(P.pos[0], P.pos[1], P.pos[2]), dRec);
    return light_intensity(L) * (invDist * invDist);
}

CTL_HD spec spot_falloff(const ctl_light_params& P, f3 d) {
    const float cosTheta = d.z;   // Frame::cosTheta
    if (cosTheta <= P.cos_cutoff_angle) return mk3s(0.0f);
    if (cosTheta >= P.cos_beam_width) return mk3s(1.0f);
    return mk3s((P.cutoff_angle - cr_acos(cosTheta)) * P.inv_transition_width);
}

CTL_HD spec spot_sample_direct(const ctl_light& L, const ctl_light_params& P, direct_rec& dRec) {
    const float invDist = delta_position_rec(mk3(P.pos[0], P.pos[1], P.pos[2]), dRec);
    spec v = light_intensity(L) * spot_falloff(P, to_local(params_frame(P), -dRec.d)) * (invDist * invDist);
    // ref == pos: the reference divides by zero and its falloff takes acos of a NaN, whose sign and
    // payload the host's and the device's libraries choose differently; every NaN leaves as the same one
    const float qnan = bits_f(0x7fc00000);
    if (v.x != v.x) v.x = qnan;
    if (v.y != v.y) v.y = qnan;
    if (v.z != v.z) v.z = qnan;
    return v;
}

// The disk centre is d * radius about the origin, as in the reference.  A reference point behind the
// disk returns 0; the record keeps what the caller put there, with pdf = 0 (the WavefrontPathTracer
// reads dRec.pdf after every sample).
CTL_HD spec distant_sample_direct(const ctl_light& L, const ctl_light_params& P, direct_rec& dRec) {
    const f3 d = to_world(params_frame(P), mk3(0.0f, 0.0f, 1.0f));
    const float radius = P.cos_beam_width;
    const f3 diskCenter = d * radius;
    const float distance = dot(dRec.ref - diskCenter, d);
    if (distance < 0) {
        dRec.pdf = 0.0f;
        return mk3s(0.0f);
    }
    dRec.p = dRec.ref - distance * d;
    dRec.d = -d;
    dRec.n = d;
    dRec.dist = distance;
    dRec.pdf = 1.0f;
    dRec.measure = kEDiscrete;
    return light_intensity(L);
}

CTL_HD float delta_pdf_direct(const direct_rec& dRec) { return dRec.measure == kEDiscrete ? 1.0f : 0.0f; }

CTL_HD bool light_is_delta(uint32_t kind) { return kind >= CTL_LIGHT_POINT && kind <= CTL_LIGHT_DISTANT; }

// What ctl_scene_upload refuses in a delta light's record (include/ctl_trace.h), for every reader of a
// scene description: null when the record and its slot are sound, else the reason.
static inline const char* delta_light_check(const ctl_light& L, const ctl_light_tri* tris, uint64_t n_tris) {
    if (L.tri_count != 0 || L.tri_first >= n_tris || !tris) return "a delta light owns one slot inside light_tris and no triangles";
    const ctl_light_params P = light_params(L, tris);
    const float* f = reinterpret_cast<const float*>(&P);
    for (int k = 0; k < 15; k++)
        if (!(fabsf(f[k]) <= FLT_MAX)) return "non-finite light parameter";
    if (!(fabsf(P.inv_transition_width) <= FLT_MAX) && !(L.kind == CTL_LIGHT_SPOT && P.inv_transition_width > 0))
        return "non-finite light parameter";
    for (int k = 0; k < 3; k++)
        if (!(fabsf(L.radiance[k]) <= FLT_MAX)) return "non-finite light intensity";
    if (L.kind != CTL_LIGHT_POINT) {
        const double n2 = (double)P.n[0] * P.n[0] + (double)P.n[1] * P.n[1] + (double)P.n[2] * P.n[2];
        if (!(fabs(sqrt(n2) - 1.0) <= 1e-5)) return "the light frame's n is not a unit vector";
    }
    if (L.kind == CTL_LIGHT_SPOT && !(P.cos_cutoff_angle <= P.cos_beam_width))
        return "spot light: cos_cutoff_angle exceeds cos_beam_width";
    return nullptr;
}

// Light::sampleDirect of lights[lidx].  ENV / DELTA: the kinds the caller's shading level carries
// (shading.h); a kind outside them falls to the area light's body, as before the kind existed.
// The environment and the area light are called where they live (ctl_env.h, ctl_shade.h).
template <bool ENV, bool DELTA>
CTL_HD spec light_sample_direct_any(const ctl_light* lights, const ctl_light_tri* tris, const float* cdfs,
                                    const EnvView& E, uint32_t lidx, direct_rec& dRec, f2 sample) {
    if (DELTA) {
        const uint32_t kind = lights[lidx].kind;
        if (light_is_delta(kind)) {
            const ctl_light L = lights[lidx];
            const ctl_light_params P = light_params(L, tris);
            if (kind == CTL_LIGHT_POINT) return point_sample_direct(L, P, dRec);
            if (kind == CTL_LIGHT_SPOT) return spot_sample_direct(L, P, dRec);
            return distant_sample_direct(L, P, dRec);
        }
    }
    return ENV && lights[lidx].kind == CTL_LIGHT_INFINITE
               ? env_sample_direct(E, dRec, sample)
               : light_sample_direct(lights[lidx], tris, cdfs, dRec, sample);
}

}  // namespace ctl
