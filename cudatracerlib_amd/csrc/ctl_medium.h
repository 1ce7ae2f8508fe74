// ctl_medium.h — one homogeneous participating medium (HomogeneousVolumeDensity,
// SceneTypes/Volumes.h:54-99) with an isotropic or a Henyey-Greenstein phase
// function, for the host scene compiler and the device kernels: fp32 in the
// reference's operation order, exp and log through cr_exp / cr_log, the sine and
// cosine of 2 pi u through cr_sin / cr_cos as ctl_bsdf.h takes them.
//
//   medium_intersect        BaseVolumeRegion::IntersectP          SceneTypes/Volumes.cu:10-20
//                           AABB::Intersect<true>                 Math/AABB.h:142-158
//   medium_tau              HomogeneousVolumeDensity::tau         SceneTypes/Volumes.cu:22-30
//   medium_transmittance    Transmittance                         Kernel/TraceAlgorithms.cu:22-31
//   medium_eval_transmittance  KernelDynamicScene::evalTransmittance  Engine/KernelDynamicScene.cu:90-96
//   medium_sample_distance  HomogeneousVolumeDensity::sampleDistance  SceneTypes/Volumes.cu:32-85
//   medium_phase_eval       KernelAggregateVolume::p              SceneTypes/Volumes.cu:307-318
//   medium_phase_sample     KernelAggregateVolume::Sample         SceneTypes/Volumes.cu:297-305
//   hg_eval / hg_sample_dir, iso_*  the two phase functions       SceneTypes/PhaseFunction.cu:9-64
//   volume_check            what upload and update refuse in a record
//
// With one volume the aggregate's IntersectP (Volumes.cu:241-255) is the
// volume's own plus `t0 < t1`, which AABB::Intersect already requires of a hit;
// a miss reports t0 = FLT_MAX, t1 = -FLT_MAX there and (0, 0) in the batch entry.
// Where the reference asks WorldBound().Contains(p) before weighting by
// sigma_s(p), the weight is already zero outside the box itself (insideWorld),
// so the box test alone decides.
#pragma once
#include "ctl_env.h"

namespace ctl {

// kepler_math::spanBeginKepler / spanEndKepler (Math/MathFunc.h:405-444): the
// two inner selections compare the floats' bit patterns as signed integers on
// both of the reference's paths.  For the bounds the integrators pass (d >= 0)
// this picks what a float comparison picks whenever the box is hit; it is kept
// so that a NaN (a ray parallel to a face and lying in its plane) takes the same
// way on the host and on the device.
CTL_HD int32_t imin_ref(int32_t a, int32_t b) { return a < b ? a : b; }
CTL_HD int32_t imax_ref(int32_t a, int32_t b) { return a > b ? a : b; }
CTL_HD float span_nan_ref(float v) { return v != v ? bits_f(0x7fc00000) : v; }
CTL_HD float span_begin_ref(float a0, float a1, float b0, float b1, float c0, float c1, float d) {
    a0 = span_nan_ref(a0); a1 = span_nan_ref(a1); b0 = span_nan_ref(b0); b1 = span_nan_ref(b1);
    c0 = span_nan_ref(c0); c1 = span_nan_ref(c1);
    const int32_t inner = imax_ref(imin_ref(f_bits(c0), f_bits(c1)), f_bits(d));              // fmin_fmax
    return bits_f(imax_ref(imax_ref(f_bits(tmin(a0, a1)), f_bits(tmin(b0, b1))), inner));     // fmax_fmax
}
CTL_HD float span_end_ref(float a0, float a1, float b0, float b1, float c0, float c1, float d) {
    a0 = span_nan_ref(a0); a1 = span_nan_ref(a1); b0 = span_nan_ref(b0); b1 = span_nan_ref(b1);
    c0 = span_nan_ref(c0); c1 = span_nan_ref(c1);
    const int32_t inner = imin_ref(imax_ref(f_bits(c0), f_bits(c1)), f_bits(d));              // fmax_fmin
    return bits_f(imin_ref(imin_ref(f_bits(tmax(a0, a1)), f_bits(tmax(b0, b1))), inner));     // fmin_fmin
}

CTL_HD m44 volume_w2v(const ctl_volume& V) { m44 m; for (int i = 0; i < 16; i++) m.d[i] = V.world_to_volume.m[i]; return m; }
CTL_HD spec volume_sig_a(const ctl_volume& V) { return mk3(V.sig_a[0], V.sig_a[1], V.sig_a[2]); }
CTL_HD spec volume_sig_s(const ctl_volume& V) { return mk3(V.sig_s[0], V.sig_s[1], V.sig_s[2]); }

// Ray * WorldToVolume (TransformPoint, TransformDirection; the direction is not
// renormalised), then the unit box with [minT, maxT] as bounds.
CTL_HD bool medium_intersect(const ctl_volume& V, f3 ori, f3 dir, float minT, float maxT, float& t0, float& t1) {
    const m44 M = volume_w2v(V);
    const f3 o = xform_point(M, ori), d = xform_dir(M, dir);
    const float tx1 = (0.0f - o.x) / d.x, tx2 = (1.0f - o.x) / d.x;
    const float ty1 = (0.0f - o.y) / d.y, ty2 = (1.0f - o.y) / d.y;
    const float tz1 = (0.0f - o.z) / d.z, tz2 = (1.0f - o.z) / d.z;
    // (a 0 / 0 here is a NaN whose sign the host's and the device's division choose
    // differently, and the sign decides the integer comparisons: span_begin_ref / span_end_ref take
    // every NaN as the positive quiet one, which is where the CUDA path's NaN sorts)
    const float mi = span_begin_ref(tx1, tx2, ty1, ty2, tz1, tz2, minT);
    const float ma = span_end_ref(tx1, tx2, ty1, ty2, tz1, tz2, maxT);
    const bool b = ma > mi && ma > 0;
    if (b) { t0 = mi; t1 = ma; }
    return b;
}

// BaseVolumeRegion::insideWorld
CTL_HD bool medium_inside(const ctl_volume& V, f3 p) {
    const f3 pl = xform_point(volume_w2v(V), p);
    return pl.x >= 0 && pl.y >= 0 && pl.z >= 0 && pl.x <= 1 && pl.y <= 1 && pl.z <= 1;
}

CTL_HD f3 ray_at(f3 ori, f3 dir, float t) { return ori + t * dir; }   // Ray::operator()

CTL_HD spec medium_tau(const ctl_volume& V, f3 ori, f3 dir, float minT, float maxT) {
    float t0, t1;
    if (!medium_intersect(V, ori, dir, minT, maxT, t0, t1)) return mk3s(0.0f);
    return length(ray_at(ori, dir, t0) - ray_at(ori, dir, t1)) * (volume_sig_a(V) + volume_sig_s(V));
}

CTL_HD spec spec_exp(spec s) { return mk3(cr_exp(s.x), cr_exp(s.y), cr_exp(s.z)); }
CTL_HD float spec_avg(spec s) { float r = 0.0f; r += s.x; r += s.y; r += s.z; return r * (1.0f / 3); }   // sum() * (1 / N)

// Transmittance(r, tmin, tmax): IntersectP, then tau over what it found.  On a
// miss the reference's a and b stay FLT_MAX and -FLT_MAX, and tau over that empty
// range misses again: 1.
CTL_HD spec medium_transmittance(const ctl_volume& V, f3 ori, f3 dir, float tmin_, float tmax_) {
    float a = FLT_MAX, b = -FLT_MAX;
    medium_intersect(V, ori, dir, tmin_, tmax_, a, b);
    return spec_exp(-medium_tau(V, ori, dir, a, b));
}

// KernelDynamicScene::evalTransmittance(p1, p2) (KernelDynamicScene.cu:90-96)
CTL_HD spec medium_eval_transmittance(const ctl_volume& V, f3 p1, f3 p2) {
    f3 d = p2 - p1;
    const float l = length(d);
    d = d / l;
    return spec_exp(-medium_tau(V, p1, d, 0.0f, l));
}

struct medium_rec {   // MediumSamplingRecord (Volumes.h:15-26) without the orientation nobody reads
    float t;
    f3 p;
    spec transmittance, sigmaA, sigmaS;
    float pdfSuccess, pdfSuccessRev, pdfFailure;
};

// t, p, sigmaA and sigmaS are written only when the sampled distance falls
// inside [minT, maxT), as in the reference.  The channel is int(rand * 3) for
// every rand in [0, 1); it is found by comparisons so that a query outside that
// range converts no out-of-range float and reads nothing outside sig_t.
CTL_HD bool medium_sample_distance(const ctl_volume& V, f3 ori, f3 dir, float minT, float maxT, float rand,
                                   medium_rec& mRec) {
    const spec sig_a = volume_sig_a(V), sig_s = volume_sig_s(V);
    // balance heuristic
    float weight = -1;
    const spec sig_t = sig_a + sig_s;
    const spec albedo = mk3(sig_s.x / sig_t.x, sig_s.y / sig_t.y, sig_s.z / sig_t.z);
    for (int i = 0; i < 3; i++)
        if (comp(albedo, i) > weight && comp(sig_t, i) != 0) weight = comp(albedo, i);
    if (weight > 0) weight = tmax(weight, 0.5f);

    float sampledDistance = FLT_MAX;
    if (rand < weight) {
        rand /= weight;
        // MonteCarlo::sampleReuse(3, rand, channel): channel = int(rand * 3), by comparisons
        const int channel = rand * 3 < 1 ? 0 : (rand * 3 < 2 ? 1 : 2);
        rand = rand * 3 - channel;
        const float samplingDensity = comp(sig_t, channel);
        sampledDistance = -cr_log(1 - rand) / samplingDensity;
    }

    bool success = true;
    if (sampledDistance < maxT - minT) {
        mRec.t = minT + sampledDistance;
        mRec.p = ray_at(ori, dir, mRec.t);
        mRec.sigmaA = sig_a;
        mRec.sigmaS = sig_s;
        if (mRec.p.x == ori.x && mRec.p.y == ori.y && mRec.p.z == ori.z) success = false;
    } else {
        sampledDistance = maxT - minT;
        success = false;
    }

    const spec tmp = spec_exp(-sig_t * sampledDistance);
    mRec.pdfFailure = spec_avg(tmp);
    mRec.pdfSuccess = spec_avg(sig_t * tmp);
    mRec.transmittance = spec_exp(sig_t * (-sampledDistance));
    mRec.pdfSuccessRev = mRec.pdfSuccess = mRec.pdfSuccess * weight;
    mRec.pdfFailure = weight * mRec.pdfFailure + (1 - weight);
    if (spec_max(mRec.transmittance) < 1e-8f) mRec.transmittance = mk3s(0.0f);
    return success;
}

#define CTL_INV_FOURPI (1.0f / (4.0f * CTL_PI))   // MathFunc.h INV_FOURPI

CTL_HD float hg_eval(float g, f3 wi, f3 wo) {
    const float temp = 1.0f + g * g + 2.0f * g * dot(wi, wo);
    return (1.0f / (4.0f * CTL_PI)) * (1 - g * g) / (temp * sqrtf(temp));
}
CTL_HD f3 hg_sample_dir(float g, f3 wi, f2 sample) {
    float cosTheta;
    if (fabsf(g) < CTL_EPSILON) {
        cosTheta = 1 - 2 * sample.x;
    } else {
        const float sqrTerm = (1 - g * g) / (1 - g + 2 * g * sample.x);
        cosTheta = (1 + g * g - sqrTerm * sqrTerm) / (2 * g);
    }
    const float sinTheta = sqrtf(1.0f - cosTheta * cosTheta);
    const float sinPhi = cr_sin(2 * CTL_PI * sample.y), cosPhi = cr_cos(2 * CTL_PI * sample.y);
    frame f;   // Frame(-wi)
    f.n = -wi;
    coordinate_system(f.n, f.s, f.t);
    return to_world(f, mk3(sinTheta * cosPhi, sinTheta * sinPhi, cosTheta));
}
CTL_HD f3 iso_sample_dir(f2 sample) {   // Warp::squareToUniformSphere
    const float z = 1.0f - 2.0f * sample.y;
    const float r = sqrtf(1.0f - z * z);
    const float sinPhi = cr_sin(2.0f * CTL_PI * sample.x), cosPhi = cr_cos(2.0f * CTL_PI * sample.x);
    return mk3(r * cosPhi, r * sinPhi, z);
}

CTL_HD float phase_eval(const ctl_volume& V, f3 wi, f3 wo) {
    return V.phase == CTL_PHASE_HG ? hg_eval(V.phase_g, wi, wo) : CTL_INV_FOURPI;
}

// KernelAggregateVolume::p: sum over the volumes that hold p of wt * f, over the sum of wt
CTL_HD float medium_phase_eval(const ctl_volume& V, f3 p, f3 wi, f3 wo) {
    float ph = 0, sumWt = 0;
    if (medium_inside(V, p)) {
        const float wt = spec_avg(volume_sig_s(V));
        sumWt += wt;
        ph += wt * phase_eval(V, wi, wo);
    }
    return sumWt != 0 ? ph / sumWt : 0.0f;
}

// KernelAggregateVolume::Sample(p, pRec(wi), pdf, sample): with one volume,
// sampleVolume asks whether the ray (p, wi) over [0, FLT_MAX] meets the box.  The
// reference tests the world bound of the box there; a point inside the medium is
// inside both, and this is called only with a point the distance sample placed in
// the medium, so the box itself is tested.  false: the weight is 0 and wo is not written.
CTL_HD bool medium_phase_sample(const ctl_volume& V, f3 p, f3 wi, f2 sample, f3& wo, float& weight, float& pdf) {
    float t0, t1;
    if (!medium_intersect(V, p, wi, 0.0f, FLT_MAX, t0, t1)) { weight = 0.0f; return false; }
    if (V.phase == CTL_PHASE_HG) {
        wo = hg_sample_dir(V.phase_g, wi, sample);
        pdf = hg_eval(V.phase_g, wi, wo);
    } else {
        wo = iso_sample_dir(sample);
        pdf = CTL_INV_FOURPI;
    }
    weight = 1.0f;
    return true;
}

// What ctl_scene_upload and ctl_scene_update refuse in a volume record
// (include/ctl_trace.h), for every reader of a scene description: null when
// the record is sound, else the reason.
static inline const char* volume_check(const ctl_volume& V) {
    if (V.kind != CTL_VOLUME_HOMOGENEOUS) return "unknown volume kind";
    if (V.phase != CTL_PHASE_ISOTROPIC && V.phase != CTL_PHASE_HG) return "unknown phase function";
    if (!(fabsf(V.phase_g) <= FLT_MAX)) return "non-finite volume field";
    for (int k = 0; k < 3; k++)
        if (!(fabsf(V.sig_a[k]) <= FLT_MAX) || !(fabsf(V.sig_s[k]) <= FLT_MAX) || !(fabsf(V.le[k]) <= FLT_MAX))
            return "non-finite volume field";
    for (int k = 0; k < 16; k++)
        if (!(fabsf(V.volume_to_world.m[k]) <= FLT_MAX) || !(fabsf(V.world_to_volume.m[k]) <= FLT_MAX))
            return "non-finite volume field";
    for (int k = 0; k < 3; k++)
        if (V.sig_a[k] < 0 || V.sig_s[k] < 0 || V.le[k] < 0) return "negative volume coefficient";
    if (!(fabsf(V.phase_g) < 1.0f)) return "the phase function's |g| must be below 1";
    return nullptr;
}

}  // namespace ctl
