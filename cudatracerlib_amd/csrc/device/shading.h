// shading.h — path shading (included by common.h): the shading levels, one statement of each
// step the reference's three integrators share (surface at a hit, emitter choice and light sample,
// emitter at a hit and its MIS weight, escaped-path term), the PathTracer's bounce shade_hit.  Only
// common.h includes it, after the definitions it uses.
#pragma once

namespace ctl {

// Loop-carried variables of PathTrace<true> (PathTracer.cu:10-33).  wo and brdf_pdf persist: diffuse_sample leaves
// them untouched when it rejects a sample, and the reference then continues with the previous values.
struct PathVars {
    spec cl, cf;
    f3 rori, rdir, last_nor, wo;
    f2 pX;
    float brdf_pdf;
    int depth;
    bool specular;
    // DifferentialGeometry partials: computed at the first hit and kept for the
    // rest of the path (PathTrace's bRec lives across bounces, PathTracer.cu:16,60-61)
    float dudx, dudy, dvdx, dvdy;
    bool has_partials;
    // kShadeMedia: the last traced ray left the scene and the path went on from a medium interaction
    // (PathTrace's r2 is then still that miss when the loop ends, PathTracer.cu:98)
    bool vol_miss;
    __device__ __forceinline__ void begin(f2 px, f3 o, f3 d) {
        dudx = dudy = dvdx = dvdy = 0.0f;
        has_partials = false;
        vol_miss = false;
        cl = mk3s(0.0f); cf = mk3s(1.0f);
        rori = o; rdir = d;
        last_nor = mk3s(0.0f);
        wo = mk3(0.0f, 0.0f, 1.0f);
        pX = px;
        brdf_pdf = 0.0f;
        depth = 0;
        specular = false;
    }
};

// NEE shadow ray of one bounce: origin = the new rori, unoccluded -> cl += add. Skipping the add for occluded /
// absent shadow rays is exact: the reference adds cf * (0 / lightPdf) = +0 there (cf is finite and >= 0).
struct ShadowReq {
    f3 d;
    float dist;
    spec add;
    bool valid;
};

// Ray-differential directions of PerspectiveSensor::sampleRayDifferential
// (Sensor.cu:130-144): rX/rY start at the camera and point through nearP + m_dx / m_dy.
__device__ __forceinline__ void sensor_diff(const DevScene& S, f2 pX, f3& o, f3& dX, f3& dY) {
    m44 s2c = to_m44(S.camera.sample_to_camera), tw = to_m44(S.camera.to_world);
    f3 nearP = xform_point(s2c, mk3(pX.x * S.camera.inv_resolution[0], pX.y * S.camera.inv_resolution[1], 0.0f));
    o = xform_point(tw, mk3s(0.0f));
    dX = xform_dir(tw, normalize(nearP + mk3(S.camera.dx[0], S.camera.dx[1], S.camera.dx[2])));
    dY = xform_dir(tw, normalize(nearP + mk3(S.camera.dy[0], S.camera.dy[1], S.camera.dy[2])));
}

// Sensor sample + primary ray of pixel (px, py) (pathKernel2, PathTracer.cu:182-194;
// PerspectiveSensor::sampleRayDifferential, Sensor.cu:130-144).  At kShadeSensors the scene's sensor
// (ctl_sensor.h; rayX and rayY are taken at the first hit, sensor_partials) consumes the aperture
// sample every other level draws and discards: the same draws in the same order.
template <int FULL = kShadeLean>
__device__ __forceinline__ f2 primary_ray(const DevScene& S, SamplerDev& rng, uint32_t px, uint32_t py, f3& o,
                                          f3& dw) {
    f2 pX = mk2((float)px, (float)py) + rng.next2();
    if constexpr (level_sensors(FULL)) {
        const f2 ap = rng.next2();
        f3 oX, dX, oY, dY;
        (void)sensor_sample_ray_differential(S.camera, scene_sensor(S), pX, ap, o, dw, oX, dX, oY, dY);
    } else {
        (void)rng.next2();   // aperture sample (unused by PerspectiveSensor)
        sensor_ray(S, pX, o, dw);
    }
    return pX;
}

// kShadeSensors: bRec.dg.computePartials(r, rX, rY) at the path's first hit with the scene's sensor.  rayX and rayY
// depend on the aperture sample, which is not carried with the path: it is the path's 2-D draw kApertureDraw, read
// again from the tables.  false (the spherical sensor, ctl_sensor.h): the path has no UV partials.
constexpr uint32_t kApertureDraw = 1;   // draw 0 is the pixel jitter
__device__ __forceinline__ bool sensor_partials(const DevScene& S, f2 pX, f2 ap, dgeom& dg) {
    f3 o, d, oX, dX, oY, dY;
    const bool has = sensor_sample_ray_differential(S.camera, scene_sensor(S), pX, ap, o, d, oX, dX, oY, dY);
    if (has) {
        compute_partials(dg, oX, dX, oY, dY);
    } else {
        dg.dudx = dg.dudy = dg.dvdx = dg.dvdy = 0.0f;
        dg.has_partials = false;
    }
    return has;
}

// Shading level of the path kernels (template FULL, DevScene::full_shading): lean = constant diffuse materials only;
// full = C5 materials (ray differentials, partials, the BSDF type switch); alpha = full plus alpha-tested traversal
// (scenes with alpha maps); env = alpha plus the environment light.  The alpha test stays out of scenes without
// alpha maps: its code in the leaf loop costs the full kernel 2 % on C5.  The environment code lives only in the env
// instantiation: inlined into the others it costs the hot kernel ~80 spilled VGPRs.  A scene with an environment map
// always runs the env level (full shading of constant diffuse materials is exact, see shade_hit).
// mat = env plus the dielectric, thindielectric, conductor, roughconductor and plastic BSDFs (ctl_bsdf.h): a scene
// with one of those types runs this level, every other scene the instantiations it ran before, whose code the five
// types do not touch.
// lights = mat plus the point, spot and distant lights (ctl_light.h) in the light sample: a scene that holds one of
// them runs this level, every other scene the instantiations it ran before.
// media = lights plus one homogeneous participating medium (ctl_medium.h): the medium step in front of the split
// into miss and hit, the attenuated light sample, the escaped-path term after a medium interaction.  A scene with a
// volume runs this level, every other scene the instantiations it ran before.
// sensors = media plus the sensor switch (ctl_sensor.h): the primary ray and the first hit's ray differentials come
// from the scene's thin-lens, orthographic, telecentric or spherical sensor.  A scene seen through another sensor
// than the perspective one runs this level, every other scene the instantiations it ran before.
// The levels, what each carries and which one a scene runs are dispatch.h's table and scene_level; the
// names below read that table: the traversal's ALPHA flag of a level, the levels that carry the environment
// light, the seven-type BSDF dispatch, the delta lights and the medium, and the instantiation the kernels
// that never trace (wavefront shade, WPT iterate) run for a level.
#define CTL_ALPHA_OF(F) (ctl::level_alpha(F))
#define CTL_ENV_OF(F) (ctl::level_env(F))
#define CTL_EXT_OF(F) (ctl::level_ext(F))
#define CTL_DELTA_LIGHTS_OF(F) (ctl::level_delta_lights(F))
#define CTL_MEDIA_OF(F) (ctl::level_media(F))
#define CTL_SENSORS_OF(F) (ctl::level_sensors(F))
#define CTL_NO_TRACE_LEVEL(F) (ctl::level_no_trace(F))
// Host: f(FU) with DevScene::full_shading as a constant (dispatch.h), over the eight levels or, for the
// kernels that never trace, the seven they instantiate.  full_shading only ever holds one of the eight
// (scene_dev.hip).  The PathTracer's kernels have their lists at their launch (path_kernels.h): the levels
// of ctl_trace.hip's code object, of path_media.hip's and of path_sensors.hip's.
template <class F>
void with_shade_level(uint32_t full, F&& f) {
    const bool known =
        with_level<kShadeLean, kShadeFull, kShadeEnv, kShadeAlpha, kShadeMat, kShadeLights, kShadeMedia, kShadeSensors>((int)full, f);
    assert(known);
    (void)known;
}
template <class F>
void with_no_trace_level(uint32_t full, F&& f) {
    const bool known =
        with_level<kShadeLean, kShadeFull, kShadeEnv, kShadeMat, kShadeLights, kShadeMedia, kShadeSensors>(
            CTL_NO_TRACE_LEVEL((int)full), f);
    assert(known);
    (void)known;
}

__device__ __forceinline__ EnvView env_view(const DevScene& S) { return EnvView{S.env, S.env_data, S.textures, S.tex_data}; }

// The surface at a hit, TraceResult::getBsdfSample (TraceResult.cu:16-45): the triangle's
// differential geometry in the node's frame (partials and b.wo are the caller's), wi, and the
// material -- its scene records (gext null below kShadeMat) and a copy -- with the two-sided flip.
// The node comes back as a pointer: a copy's lights[] would be indexed dynamically, i.e. in scratch.
// hit_geometry is its TriangleData::fillDG part, for a kernel that keeps the rest written out (wpt.hip).
__device__ __forceinline__ void hit_geometry(const DevScene& S, uint32_t node, const ctl_triangle_data& td, f2 bary,
                                             f3 P, bool half_quirk, dgeom& dg) {
    dg.P = P;
    fill_dg(td, load_m44(S.xf + 4 * node), bary, half_quirk, LutDecode{S.normal_lut}, dg);
}
struct HitSurface {
    const ctl_node* N;
    const ctl_material* gmat;
    const ctl_material_ext* gext;
};
template <int FULL>
__device__ __forceinline__ ctl_material surface_at(const DevScene& S, uint32_t node, uint32_t tri, f2 bary, f3 P,
                                                   f3 dir, bool half_quirk, dgeom& dg, bsdf_rec& b, HitSurface& sf) {
    b.sampled_type = 0; b.type_mask = kEAll;
    const ctl_triangle_data td = S.tri_data[tri];
    sf.N = S.nodes + node;
    hit_geometry(S, node, td, bary, P, half_quirk, dg);
    b.wi = to_local(dg.sys, -dir);
    const uint32_t mat_index = material_index(S, td, node);
    sf.gmat = S.mats + mat_index;
    sf.gext = CTL_EXT_OF(FULL) ? S.mats_ext + mat_index : nullptr;
    const ctl_material mat = *sf.gmat;
    if (mat.two_sided && b.wi.z < 0) { dg.n = -dg.n; dg.sys.n = -dg.sys.n; b.wi.z *= -1.0f; }
    return mat;
}

// A diffuse (at kShadeMat also plastic) hit with a reflectance texture: one lookup for BSDF sample and NEE
template <int FULL>
__device__ __forceinline__ bool textured_reflectance(const ctl_material& mat) {
    return FULL && (mat.bsdf_type == CTL_BSDF_DIFFUSE || (CTL_EXT_OF(FULL) && mat.bsdf_type == CTL_BSDF_PLASTIC)) &&
           mat.texture != 0xffffffffu;
}

// KernelDynamicScene::pdfEmitter (KernelDynamicScene.cu:42-46)
__device__ __forceinline__ float pdf_emitter(const DevScene& S, uint32_t li) {
    return S.light_cdf[li] - (li == 0 ? 0.0f : S.light_cdf[li - 1]);
}

// KernelDynamicScene::sampleEmitter (KernelDynamicScene.cu:25-39; needs S.n_lights > 0): the
// light sample.x picks, sample.x rescaled to that light's interval, and the pick's probability.
__device__ __forceinline__ uint32_t sample_emitter(const DevScene& S, f2& sample, float& emPdf) {
    const uint32_t nl = S.n_lights < CTL_MAX_NUM_LIGHTS ? S.n_lights : CTL_MAX_NUM_LIGHTS;
    uint32_t first = 0, cnt = nl;   // STL_upper_bound
    while (cnt > 0) {
        uint32_t c2 = cnt / 2, mid = first + c2;
        if (!(sample.x < S.light_cdf[mid])) { first = mid + 1; cnt -= c2 + 1; }
        else cnt = c2;
    }
    const uint32_t idx = first < nl ? first : nl - 1;
    const float fU = S.light_cdf[idx], fL = idx > 0 ? S.light_cdf[idx - 1] : 0.0f;
    sample.x = (sample.x - fL) / (fU - fL);
    emPdf = fU - fL;
    return idx;
}

// Light::sampleDirect dispatch (ctl_light.h): the kinds the level carries, else a diffuse area light
template <int FULL>
__device__ __forceinline__ spec sample_light_direct(const DevScene& S, uint32_t lidx, direct_rec& dRec, f2 sample) {
    return light_sample_direct_any<CTL_ENV_OF(FULL), CTL_DELTA_LIGHTS_OF(FULL)>(S.lights, S.light_tris, S.light_tri_cdf,
                                                                                env_view(S), lidx, dRec, sample);
}

// The emitter of a hit whose material has one (mat.node_light_index set): index, record, and
// TraceResult::Le(p, sys, w) -> DiffuseLight::eval (Light.cu:67-82), zero seen from behind.
struct HitEmitter {
    uint32_t li;
    ctl_light L;
    __device__ __forceinline__ HitEmitter(const DevScene& S, const ctl_node* N, const ctl_material& mat)
        : li(N->lights[mat.node_light_index]), L(S.lights[li]) {}
    __device__ __forceinline__ spec Le(const dgeom& dg, f3 w) const {
        return (dot(dg.sys.n, w) <= 0) ? mk3s(0.0f) : mk3(L.radiance[0], L.radiance[1], L.radiance[2]);
    }
};

// MIS weight of that radiance against the BSDF sample that found it (PathTracer.cu:66-72,
// WavefrontPathTracer.cu:96-101): DirectSamplingRecFromRay from (ref, refN) along d to the hit.
__device__ __forceinline__ float emitter_mis(const DevScene& S, const HitEmitter& E, f3 ref, f3 refN, const dgeom& dg,
                                             f3 d, float dist, float bsdf_pdf) {
    direct_rec dRec;
    dRec.ref = ref; dRec.refN = refN; dRec.p = dg.P; dRec.n = dg.n;
    dRec.d = d; dRec.dist = dist; dRec.measure = kESolidAngle;
    const float direct_pdf = light_pdf_direct(E.L, dRec) * pdf_emitter(S, E.li);
    return power_heuristic(bsdf_pdf, direct_pdf);
}

// The escaped-path term of PathTrace (PathTracer.cu:98-111):
// misWeight * cf * EvalEnvironment(r), with r the last traced ray.  Without an
// environment map EvalEnvironment is 0 and the sum stays as it was.
template <int FULL>
__device__ __forceinline__ spec env_miss(const DevScene& S, const PathParams& P, const PathVars& v) {
    if (!CTL_ENV_OF(FULL) || S.env_index == 0xffffffffu) return (v.cf * 1.0f) * mk3s(0.0f);
    const EnvView E = env_view(S);
    float misWeight = 1.0f;
    if (!(!P.direct || v.depth == 1 || v.specular)) {
        direct_rec dRec;   // DirectSamplingRecFromRay: d = r.dir, solid-angle measure
        dRec.d = v.rdir; dRec.measure = kESolidAngle;
        dRec.ref = v.rori; dRec.refN = v.last_nor; dRec.p = mk3s(0.0f); dRec.n = mk3s(0.0f); dRec.dist = 0.0f;
        const float direct_pdf = env_pdf_direct(E, dRec) * pdf_emitter(S, S.env_index);
        misWeight = power_heuristic(v.brdf_pdf, direct_pdf);
    }
    return (v.cf * misWeight) * env_eval(E, v.rdir);
}

// Transmittance(ray, t0, t1) of the scene's medium (kShadeMedia and above).  kShadeSensors also runs scenes
// without a medium, whose record is all zero (kind 0): there the factor is the 1 the lower levels multiply by.
template <int FULL>
__device__ __forceinline__ spec scene_transmittance(const DevScene& S, f3 o, f3 d, float t0, float t1) {
    const ctl_volume& V = scene_volume(S);
    if constexpr (CTL_SENSORS_OF(FULL)) { if (V.kind == 0) return mk3s(1.0f); }
    return medium_transmittance(V, o, d, t0, t1);
}

// UniformSampleOneLight up to its occlusion test (TraceAlgorithms.cu:44-73, 92-101; needs S.n_lights > 0): draws the
// light choice and the light position, and when both the light sample and the BSDF value are non-zero fills the
// shadow ray and, in sh.add, EstimateDirect(...) / pdf -- the value UniformSampleOneLight returns when the shadow
// ray is unoccluded (it returns +0 otherwise).  gm: the material's record in the scene array (the rough-dielectric
// calls read it there; required for FULL), R: the diffuse reflectance when already evaluated (or null).
// ATT: EstimateDirect's `attenuated` -- the PathTracer passes true, the PrimTracer its default false
// (PrimTracer.cu:67) -- which only a level with a medium can tell from false.
template <int FULL, bool ATT = CTL_MEDIA_OF(FULL)>
__device__ __forceinline__ void nee_sample(const DevScene& S, SamplerDev& rng, const ctl_material& mat,
                                           const bsdf_rec& b, const dgeom& dg, const TexView& tex, ShadowReq& sh,
                                           const spec* R, const ctl_material* gm,
                                           const ctl_material_ext* ge = nullptr) {
    f2 sample = rng.next2();
    float lpdf;
    const uint32_t lidx = sample_emitter(S, sample, lpdf);
    direct_rec dRec;
    dRec.p = dg.P; dRec.n = dg.sys.n; dRec.measure = kEArea;
    dRec.ref = dg.P; dRec.refN = dg.sys.n;
    spec value = sample_light_direct<FULL>(S, lidx, dRec, rng.next2());
    if (!spec_zero(value)) {
        bsdf_rec b2 = b;
        b2.wo = to_local(dg.sys, dRec.d);
        b2.type_mask = kEAll & ~kEDelta;
        spec bsdfVal = FULL ? bsdf_f<CTL_EXT_OF(FULL)>(mat, b2, dg, &tex, R, gm, ge) : diffuse_f(mat, b2);
        if (!spec_zero(bsdfVal)) {
            float weight = 1.0f;
            if (dRec.measure != kEDiscrete)
                weight = power_heuristic(dRec.pdf * lpdf, FULL ? bsdf_pdf<CTL_EXT_OF(FULL)>(mat, b2, gm, ge) : diffuse_pdf(mat, b2));
            spec ret = value * bsdfVal * weight;
            if constexpr (ATT) ret = ret * scene_transmittance<FULL>(S, dRec.ref, dRec.d, 0.0f, dRec.dist);
            else ret = ret * mk3s(1.0f);
            sh.valid = true;
            sh.d = dRec.d;
            sh.dist = dRec.dist;
            sh.add = spec_div(ret, lpdf);
        }
    }
}

// The medium in front of PathTrace's split into miss and hit (PathTracer.cu:24-58, kShadeMedia only): h is the
// traced ray's result (t = FLT_MAX on a miss).
//   kMediumNone       no interaction: the ray does not meet the medium, or the distance sample failed; a hit behind
//                     the medium then carries cf * transmittance / pdfFailure and is shaded as ever, a miss ends the
//                     path through env_miss unweighted.
//   kMediumScattered  cf *= sigmaS * transmittance / pdfSuccess; the light sample from the medium point
//                     (sampleAttenuatedEmitterDirect, KernelDynamicScene.cu:98-123: ONE 2-D draw shared by the emitter
//                     choice and the light position, the transmittance to the light folded into sh.add, the power
//                     heuristic whatever the light's measure) left in sh; the phase sample; the path goes on from the
//                     medium point.  specular, brdf_pdf and last_nor keep their values, as in the reference.
//   kMediumEnded      the same, and Russian roulette (:91-96) ended the path.
// The distance is sampled over the clipped [minT, maxT], not over [0, h.t] (include/ctl_trace.h, ctl_volume).
// Sampler draws in the reference's order: distance 1D, light 2D, phase 2D, RR 1D.
enum : int { kMediumNone = 0, kMediumScattered = 1, kMediumEnded = 2 };
template <int FULL>
__device__ __forceinline__ int medium_step(const DevScene& S, const PathParams& P, SamplerDev& rng, PathVars& v,
                                           const HitRec& h, ShadowReq& sh) {
    sh.valid = false;
    const ctl_volume& V = scene_volume(S);   // one record for every lane, at a kernel-uniform address
    // kShadeSensors also runs scenes without a medium (an all-zero record): no interaction, no draw
    if constexpr (CTL_SENSORS_OF(FULL)) { if (V.kind == 0) return kMediumNone; }
    float minT, maxT;
    if (!medium_intersect(V, v.rori, v.rdir, 0.0f, h.t, minT, maxT)) return kMediumNone;
    medium_rec m;
    if (!medium_sample_distance(V, v.rori, v.rdir, minT, maxT, rng.next1(), m)) {
        if (h.tri != 0xffffffffu) v.cf = v.cf * spec_div(m.transmittance, m.pdfFailure);
        return kMediumNone;
    }
    v.cf = v.cf * spec_div(m.sigmaS * m.transmittance, m.pdfSuccess);
    const f3 wi = -v.rdir;
    if (P.direct) {
        f2 sample = rng.next2();
        if (S.n_lights) {
            direct_rec dRec;   // DirectSamplingRecord(mRec.p, 0); sampleEmitterDirect clears pdf
            dRec.ref = m.p; dRec.refN = mk3s(0.0f); dRec.p = m.p; dRec.n = mk3s(0.0f);
            dRec.d = mk3s(0.0f); dRec.dist = 0.0f; dRec.pdf = 0.0f; dRec.measure = kEArea;
            float emPdf;
            const uint32_t lidx = sample_emitter(S, sample, emPdf);
            spec value = sample_light_direct<FULL>(S, lidx, dRec, sample);
            if (dRec.pdf != 0) {
                dRec.pdf *= emPdf;
                value = spec_div(value, emPdf);
            } else {
                value = mk3s(0.0f);
            }
            value = value * medium_eval_transmittance(V, dRec.ref, dRec.p);
            if (!spec_zero(value)) {
                const float p = medium_phase_eval(V, m.p, wi, dRec.d);
                if (p != 0) {
                    const float weight = power_heuristic(dRec.pdf, p);
                    sh.valid = true;
                    sh.d = dRec.d;
                    sh.dist = dRec.dist;
                    sh.add = ((v.cf * value) * p) * weight;
                }
            }
        }
    }
    f3 wo;
    float w, pdf;
    // a weight of 0 (the point is not in the medium after all) leaves wo unwritten in the reference;
    // the direction stays, and cf = 0 makes every later term of the path +0
    if (medium_phase_sample(V, m.p, wi, rng.next2(), wo, w, pdf)) v.rdir = wo;
    v.cf = v.cf * w;
    v.rori = m.p;
    if (v.depth > P.rr_start_depth && !v.specular) {
        if (rng.next1() >= spec_max(v.cf)) return kMediumEnded;
        v.cf = spec_div(v.cf, spec_max(v.cf));
    }
    return kMediumScattered;
}

// One closest hit of PathTrace<DIRECT> (PathTracer.cu:35-96; DIRECT = P.direct): emission with MIS, BSDF sample,
// UniformSampleOneLight up to its occlusion test (TraceAlgorithms.cu:44-73, 92-101; sampleEmitter
// KernelDynamicScene.cu:25-39), throughput update and Russian roulette.  Returns false when RR ends the path.
// Sampler draws are in the reference order: BSDF 2D, light choice 2D, light position 2D, RR 1D.
// FULL = the scene has C5 materials (roughdielectric or image textures): ray differentials, partials and the BSDF
// type switch.  Scenes with constant diffuse materials only take the lean instantiation — the partials are only
// observable through textures, so both give identical results there.
// SINGLE: one-instance scene, so the hit's node is ~start_node for every lane; indexing with that kernel-uniform
// value turns the node record and its transform into scalar loads.
// part: when non-null (persistent kernel), the path's first-hit partials live in this memory slot instead of
// PathVars, so they hold no VGPRs across the traces; they are read back only for a textured material, the one
// consumer of the partials.  has_partials is then `depth > 1` (the first hit always computes them); at kShadeMedia
// the depth-1 event can be a medium interaction, so there the loop keeps v.has_partials itself.
// pk: when non-null (persistent kernel, PK = its LDS park), the path variables other than the ray, depth / specular
// and the sampler state are still parked in LDS on entry and are read where they are used: pX for the first-hit
// partials, brdf_pdf and last_nor for an emitter's MIS weight, wo and brdf_pdf just before the BSDF sample, cl and
// cf at the end.  So they hold no VGPRs across the out-of-line texture and microfacet calls.  The arithmetic is the
// same either way.
struct NoPark {};
template <int FULL, bool SINGLE = false, class PK = NoPark>
__device__ __forceinline__ bool shade_hit(const DevScene& S, const PathParams& P, SamplerDev& rng, PathVars& v,
                                          const HitRec& r, ShadowReq& sh, float4* part = nullptr,
                                          const PK* pk = nullptr) {
    constexpr bool kLazy = !std::is_same<PK, NoPark>::value;
    const uint32_t node = SINGLE ? ~(uint32_t)S.start_node : r.node;
    sh.valid = false;
    bsdf_rec b;
    dgeom dg;
    HitSurface sf;
    // surface_at's steps written out: as a call, the path kernels' registers and spills change
    b.sampled_type = 0; b.type_mask = kEAll;
    dg.P = v.rori + r.t * v.rdir;
    const ctl_triangle_data td = S.tri_data[r.tri];
    sf.N = S.nodes + node;
    fill_dg(td, load_m44(S.xf + 4 * node), mk2(r.u, r.v), P.half_quirk, LutDecode{S.normal_lut}, dg);
    b.wi = to_local(dg.sys, -v.rdir);
    const uint32_t mat_index = material_index(S, td, node);
    sf.gmat = S.mats + mat_index;
    sf.gext = CTL_EXT_OF(FULL) ? S.mats_ext + mat_index : nullptr;
    const ctl_material mat = *sf.gmat;
    if (mat.two_sided && b.wi.z < 0) { dg.n = -dg.n; dg.sys.n = -dg.sys.n; b.wi.z *= -1.0f; }
    if (FULL) {
        if (v.depth == 1) {   // bRec.dg.computePartials(r, rX, rY) (PathTracer.cu:60-61)
            if constexpr (kLazy) pk->load_px(v);
            bool has = true;   // kShadeSensors: the sensor defines rayX and rayY (sensor_partials)
            if constexpr (CTL_SENSORS_OF(FULL)) {
                has = sensor_partials(S, v.pX, rng.peek2(kApertureDraw), dg);
            } else {
                f3 co, dX, dY;
                sensor_diff(S, v.pX, co, dX, dY);
                compute_partials(dg, co, dX, co, dY);
            }
            if (part) {
                *part = make_float4(dg.dudx, dg.dudy, dg.dvdx, dg.dvdy);
                if constexpr (CTL_MEDIA_OF(FULL)) v.has_partials = has;
            } else {
                v.dudx = dg.dudx; v.dudy = dg.dudy; v.dvdx = dg.dvdx; v.dvdy = dg.dvdy;
                v.has_partials = has;
            }
        } else if (part) {
            // kShadeMedia: a path whose depth-1 event was a medium interaction meets its first surface here with
            // nothing in the slot; bRec.dg then still has hasUVPartials = false and no partials (v.has_partials,
            // a register of the persistent loop at this level only)
            const bool written = CTL_MEDIA_OF(FULL) ? v.has_partials : true;
            dg.has_partials = written;
            float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (written && mat.texture != 0xffffffffu) q = *part;
            dg.dudx = q.x; dg.dudy = q.y; dg.dvdx = q.z; dg.dvdy = q.w;
        } else {
            dg.dudx = v.dudx; dg.dudy = v.dudy; dg.dvdx = v.dvdx; dg.dvdy = v.dvdy;
            dg.has_partials = v.has_partials;
        }
    }
    const TexView tex{S.textures, S.tex_data};
    if (mat.node_light_index != 0xffffffffu) {
        const HitEmitter E(S, sf.N, mat);
        float misWeight = 1.0f;
        if (!(!P.direct || v.depth == 1 || v.specular)) {   // PathTracer.cu:66-67
            if constexpr (kLazy) pk->load_mis(v);
            // emitter_mis written out: as a call, the persistent kernels' registers and spills change
            direct_rec dRec;
            dRec.ref = v.rori; dRec.refN = v.last_nor; dRec.p = dg.P; dRec.n = dg.n;
            dRec.d = v.rdir; dRec.dist = r.t; dRec.measure = kESolidAngle;
            float direct_pdf = light_pdf_direct(E.L, dRec) * pdf_emitter(S, E.li);
            misWeight = power_heuristic(v.brdf_pdf, direct_pdf);
        }
        const spec Le = E.Le(dg, -v.rdir);
        if constexpr (kLazy) pk->load_cl_cf(v);
        v.cl = v.cl + (v.cf * misWeight) * Le;
        if constexpr (kLazy) pk->store_cl(v);
    }
    // The diffuse reflectance is evaluated here for every diffuse hit (refl(mat)
    // when untextured, the value diffuse_reflectance returns) and handed to the
    // BSDF sample and the NEE evaluation, so the full kernel has one texture
    // call site instead of three (C5 kernel VGPR spills 27 -> 24).
    spec Rtex = refl(mat);
    if (textured_reflectance<FULL>(mat)) Rtex = diffuse_reflectance(mat, dg, &tex);
    const spec* Rp = FULL ? &Rtex : nullptr;
    if constexpr (kLazy) pk->load_sample_state(v);
    b.wo = v.wo;
    spec f = FULL ? bsdf_sample<CTL_EXT_OF(FULL)>(mat, b, v.brdf_pdf, rng.next2(), dg, &tex, Rp, sf.gmat, sf.gext)
                  : diffuse_sample(mat, b, v.brdf_pdf, rng.next2());
    v.last_nor = dg.sys.n;
    if (P.direct && (mat.combined_type & kESmooth) != 0 && S.n_lights) {   // PathTracer.cu:82-83
        nee_sample<FULL>(S, rng, mat, b, dg, tex, sh, Rp, sf.gmat, sf.gext);
    }
    if constexpr (kLazy) pk->load_cl_cf(v);
    if (sh.valid) sh.add = v.cf * sh.add;
    v.specular = (b.sampled_type & kEDelta) != 0;
    v.cf = v.cf * f;
    v.rori = dg.P;
    v.rdir = to_world(dg.sys, b.wo);
    v.wo = b.wo;
    if (v.depth > P.rr_start_depth && !v.specular) {
        if (rng.next1() >= spec_max(v.cf)) return false;
        v.cf = spec_div(v.cf, spec_max(v.cf));
    }
    return true;
}

// KernelDynamicScene::Occluded(ray, 0, dist) decided from a finished shadow traversal (KernelDynamicScene.cu:70-80):
// any-hit over (eps, dist - eps), or the reference's closest hit tested against (eps, dist - eps), where a miss with
// an infinite dist is not occluded (:77-78).
__device__ __forceinline__ bool shadow_occluded(const DevScene& S, bool any_hit, const HitRec& h, float dist) {
    if (any_hit) return h.tri != 0xffffffffu;
    bool end = h.t < dist - S.ray_eps;
    if (isinf(dist) && h.tri == 0xffffffffu) end = false;
    return h.t > 0 + S.ray_eps && end;
}
// The any-hit shadow query over (eps, dist - eps) culls boxes at dist + slab_slack(ray) (traverse.h), not at its
// acceptance bound: a box whose rounded slab entry lands past dist - eps, or past dist (the slab cancels two
// products of size |o| |idir|), can hold a hit below dist - eps, which the reference's closest-hit query finds (it
// culls nothing before its first hit). tests/test_shadow_query.py measures the rules against the reference's form.

}  // namespace ctl
