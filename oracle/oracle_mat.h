// oracle_mat.h — TEST INFRASTRUCTURE ONLY (part of oracle.cpp).
//
// CPU restatement of the reference's dielectric, thindielectric, conductor,
// roughconductor and plastic BSDFs, for checking the device path bit for bit.
// Written from the reference, in its operation order:
//   Math/FresnelHelper.h       fresnelConductorExact (Spectrum)        :119-142
//   Math/Frame.h               reflect, refract (local)                :138-156
//   Math/Warp.h                squareToCosineHemisphere(+Pdf), disk    :61-71, 102-125
//   Math/Spectrum.h            operator/ (Scalar) = * (1 / f)          :122-128, 150-155
//   SceneTypes/Dispersion.h    DispersionCauchy with C = 0             :26-29, 125-168
//   SceneTypes/BSDF_Simple.cu  dielectric                              :174-277
//                              thindielectric                          :279-371
//                              conductor                               :617-660
//                              roughconductor                          :662-763
//                              plastic                                 :765-888
// The parameters come from ctl_material and ctl_material_ext as
// include/ctl_trace.h lays them out.  Included by oracle.cpp after
// oracle_c5.h and diffuse_R; uses the oracle's own V3 / Spec / BRec.
#pragma once

namespace omat {

using namespace oracle;

const float DeltaEpsilon = 1e-3f;   // MathFunc.h:26
const int MSolidAngle = 1, MDiscrete = 4;   // EMeasure (SceneTypes/Samples.h)

inline Spec sdiv(Spec a, Spec b) { return v3(a.x / b.x, a.y / b.y, a.z / b.z); }   // Spectrum.h:115-120
inline Spec ssafe_sqrt(Spec a) { return v3(c5::safe_sqrt(a.x), c5::safe_sqrt(a.y), c5::safe_sqrt(a.z)); }

// FresnelHelper::fresnelConductorExact(float, Spectrum, Spectrum) (FresnelHelper.h:119-142)
inline Spec fresnel_conductor_exact(float cosThetaI, Spec eta, Spec k) {
    float cosThetaI2 = cosThetaI * cosThetaI, sinThetaI2 = 1 - cosThetaI2, sinThetaI4 = sinThetaI2 * sinThetaI2;
    Spec temp1 = eta * eta - k * k - v3s(sinThetaI2), a2pb2 = ssafe_sqrt(temp1 * temp1 + k * k * eta * eta * 4.0f),
         a = ssafe_sqrt((a2pb2 + temp1) * 0.5f);
    Spec term1 = a2pb2 + v3s(cosThetaI2), term2 = a * (2 * cosThetaI);
    Spec Rs2 = sdiv(term1 - term2, term1 + term2);
    Spec term3 = a2pb2 * cosThetaI2 + v3s(sinThetaI4), term4 = term2 * sinThetaI2;
    Spec Rp2 = sdiv(Rs2 * (term3 - term4), term3 + term4);
    return 0.5f * (Rp2 + Rs2);
}

inline V3 frame_reflect(V3 wi) { return v3(-wi.x, -wi.y, wi.z); }   // Frame.h:138-145
inline V3 frame_refract(V3 wi, float cosThetaT, float eta, float invEta) {   // Frame.h:148-156, normalized
    float scale = -(cosThetaT < 0 ? invEta : eta);
    return normalize(v3(scale * wi.x, scale * wi.y, cosThetaT));
}

// Warp::squareToCosineHemisphere over squareToUniformDiskConcentric (Warp.h:61-66, 102-125)
inline V3 cosine_hemisphere(V2 sample) {
    float r1 = 2.0f * sample.x - 1.0f, r2 = 2.0f * sample.y - 1.0f;
    float phi, r;
    if (r1 == 0 && r2 == 0) { r = phi = 0; }
    else if (r1 * r1 > r2 * r2) { r = r1; phi = (O_PI / 4.0f) * (r2 / r1); }
    else { r = r2; phi = (O_PI / 2.0f) - (r1 / r2) * (O_PI / 4.0f); }
    float sinPhi = cr_sin(phi), cosPhi = cr_cos(phi);
    V2 p = v2(r * cosPhi, r * sinPhi);
    float z = sqrtf(1.0f - p.x * p.x - p.y * p.y);
    return v3(p.x, p.y, z);
}
inline float cosine_hemisphere_pdf(V3 d) { return O_INV_PI * d.z; }   // Warp.h:68-71

inline Spec ext_eta(const ctl_material_ext& e) { return v3(e.eta[0], e.eta[1], e.eta[2]); }
inline Spec ext_k(const ctl_material_ext& e) { return v3(e.k[0], e.k[1], e.k[2]); }
inline Spec ext_specular(const ctl_material_ext& e) { return v3(e.specular[0], e.specular[1], e.specular[2]); }

// ---------------------------------------------------------------- dielectric
// eta_f is a DispersionCauchy(B = eta, C = 0): hasDispersion() is false, so
// sample_eta / f_eta / pdf_eta give f_o = 1, pdf = 1 and calc_eta(600).
inline float cauchy_eta(const ctl_material& m) { return m.eta + 0.0f / (600.0f / 1e3f); }

// events (may be null): [0] counts a sample whose Fresnel term reported total
// internal reflection from inside (wi.z < 0, cosThetaT = 0)
inline Spec dielectric_sample(const ctl_material& m, BRec& b, float& pdf, V2 sample, uint64_t* tir) {
    bool sampleReflection = (b.typeMask & CTL_EDELTA_REFLECTION) != 0;
    bool sampleTransmission = (b.typeMask & CTL_EDELTA_TRANSMISSION) != 0;
    Spec f_o = v3s(1.0f);
    float cosThetaT, eta_pdf = 1.0f, eta = cauchy_eta(m), invEta = 1.0f / eta;
    float F = c5::fresnel_ext(b.wi.z, cosThetaT, eta);
    if (sampleTransmission && sampleReflection) {
        if (sample.x <= F) {
            if (tir && b.wi.z < 0 && cosThetaT == 0.0f && F == 1.0f) (*tir)++;
            b.sampledType = CTL_EDELTA_REFLECTION;
            b.wo = frame_reflect(b.wi);
            pdf = F;
            return c5::spec_refl(m);
        } else {
            b.sampledType = CTL_EDELTA_TRANSMISSION;
            b.wo = frame_refract(b.wi, cosThetaT, eta, invEta);
            pdf = (1 - F) * eta_pdf;
            float factor = cosThetaT < 0 ? invEta : eta;   // ERadiance
            return f_o * c5::spec_trans(m) * (factor * factor);
        }
    } else if (sampleReflection) {
        b.sampledType = CTL_EDELTA_REFLECTION;
        b.wo = frame_reflect(b.wi);
        pdf = 1.0f;
        return c5::spec_refl(m);
    } else if (sampleTransmission) {
        b.sampledType = CTL_EDELTA_TRANSMISSION;
        b.wo = frame_refract(b.wi, cosThetaT, eta, invEta);
        pdf = 1.0f * eta_pdf;
        float factor = cosThetaT < 0 ? invEta : eta;
        return f_o * c5::spec_trans(m) * (factor * factor * (1 - F));
    }
    return v3s(0.0f);
}

inline Spec dielectric_f(const ctl_material& m, const BRec& b, int measure) {
    bool sampleReflection = (b.typeMask & CTL_EDELTA_REFLECTION) && measure == MDiscrete;
    bool sampleTransmission = (b.typeMask & CTL_EDELTA_TRANSMISSION) && measure == MDiscrete;
    Spec f_o = v3s(1.0f);
    float eta = cauchy_eta(m), invEta = 1.0f / eta;
    float cosThetaT;
    float F = c5::fresnel_ext(b.wi.z, cosThetaT, eta);
    if (b.wi.z * b.wo.z >= 0) {
        if (!sampleReflection || fabsf(dot(frame_reflect(b.wi), b.wo) - 1) > DeltaEpsilon) return v3s(0.0f);
        return c5::spec_refl(m) * F;
    } else {
        if (!sampleTransmission || fabsf(dot(frame_refract(b.wi, cosThetaT, eta, invEta), b.wo) - 1) > DeltaEpsilon)
            return v3s(0.0f);
        float factor = cosThetaT < 0 ? invEta : eta;
        return f_o * c5::spec_trans(m) * factor * factor * (1 - F);
    }
}

inline float dielectric_pdf(const ctl_material& m, const BRec& b, int measure) {
    bool sampleReflection = (b.typeMask & CTL_EDELTA_REFLECTION) && measure == MDiscrete;
    bool sampleTransmission = (b.typeMask & CTL_EDELTA_TRANSMISSION) && measure == MDiscrete;
    float eta_pdf = 1.0f;
    float eta = cauchy_eta(m), invEta = 1.0f / eta;
    float cosThetaT;
    float F = c5::fresnel_ext(b.wi.z, cosThetaT, eta);
    if (b.wi.z * b.wo.z >= 0) {
        if (!sampleReflection || fabsf(dot(frame_reflect(b.wi), b.wo) - 1) > DeltaEpsilon) return 0.0f;
        return sampleTransmission ? eta_pdf * F : 1.0f;
    } else {
        if (!sampleTransmission || fabsf(dot(frame_refract(b.wi, cosThetaT, eta, invEta), b.wo) - 1) > DeltaEpsilon)
            return 0.0f;
        return sampleReflection ? 1 - F : eta_pdf * 1.0f;
    }
}

// ---------------------------------------------------------------- thindielectric
inline V3 transmit(V3 wi) { return -wi; }   // BSDF_Simple.h:119-121
inline float thin_R(const ctl_material& m, const BRec& b) {   // R' = R + TRT + TR^3T + ..
    float R = c5::fresnel_ext(fabsf(b.wi.z), m.eta), T = 1 - R;
    if (R < 1) R += T * T * R / (1 - R * R);
    return R;
}

inline float thin_pdf(const ctl_material& m, const BRec& b, int measure) {
    bool sampleReflection = (b.typeMask & CTL_EDELTA_REFLECTION) && measure == MDiscrete;
    bool sampleTransmission = (b.typeMask & CTL_ENULL) && measure == MDiscrete;
    float R = thin_R(m, b);
    if (b.wi.z * b.wo.z >= 0) {
        if (!sampleReflection || fabsf(dot(frame_reflect(b.wi), b.wo) - 1) > DeltaEpsilon) return 0.0f;
        return sampleTransmission ? R : 1.0f;
    } else {
        if (!sampleTransmission || fabsf(dot(transmit(b.wi), b.wo) - 1) > DeltaEpsilon) return 0.0f;
        return sampleReflection ? 1 - R : 1.0f;
    }
}

inline Spec thin_f(const ctl_material& m, const BRec& b, int measure) {
    bool sampleReflection = (b.typeMask & CTL_EDELTA_REFLECTION) && measure == MDiscrete;
    bool sampleTransmission = (b.typeMask & CTL_ENULL) && measure == MDiscrete;
    float R = thin_R(m, b);
    if (b.wi.z * b.wo.z >= 0) {
        if (!sampleReflection || fabsf(dot(frame_reflect(b.wi), b.wo) - 1) > DeltaEpsilon) return v3s(0.0f);
        return c5::spec_refl(m) * R;
    } else {
        if (!sampleTransmission || fabsf(dot(transmit(b.wi), b.wo) - 1) > DeltaEpsilon) return v3s(0.0f);
        return c5::spec_trans(m) * (1 - R);
    }
}

inline Spec thin_sample(const ctl_material& m, BRec& b, float& pdf, V2 sample) {
    bool sampleReflection = (b.typeMask & CTL_EDELTA_REFLECTION) != 0;
    bool sampleTransmission = (b.typeMask & CTL_ENULL) != 0;
    float R = thin_R(m, b);
    if (sampleTransmission && sampleReflection) {
        if (sample.x <= R) {
            b.sampledType = CTL_EDELTA_REFLECTION;
            b.wo = frame_reflect(b.wi);
            pdf = R;
            return c5::spec_refl(m);
        } else {
            b.sampledType = CTL_ENULL;
            b.wo = transmit(b.wi);
            pdf = 1 - R;
            return c5::spec_trans(m);
        }
    } else if (sampleReflection) {
        b.sampledType = CTL_EDELTA_REFLECTION;
        b.wo = frame_reflect(b.wi);
        pdf = 1.0f;
        return c5::spec_refl(m) * R;
    } else if (sampleTransmission) {
        b.sampledType = CTL_ENULL;
        b.wo = transmit(b.wi);
        pdf = 1.0f;
        return c5::spec_trans(m) * (1 - R);
    }
    return v3s(0.0f);
}

// ---------------------------------------------------------------- conductor
inline Spec conductor_sample(const ctl_material& m, const ctl_material_ext& e, BRec& b, float& pdf, V2) {
    bool sampleReflection = (b.typeMask & CTL_EDELTA_REFLECTION) != 0;
    if (!sampleReflection || b.wi.z <= 0) return v3s(0.0f);
    b.sampledType = CTL_EDELTA_REFLECTION;
    b.wo = frame_reflect(b.wi);
    pdf = 1;
    return c5::spec_refl(m) * fresnel_conductor_exact(b.wi.z, ext_eta(e), ext_k(e));
}
inline bool conductor_pair(const BRec& b, int measure) {
    bool sampleReflection = (b.typeMask & CTL_EDELTA_REFLECTION) != 0;
    return !(!sampleReflection || measure != MDiscrete || b.wi.z <= 0 || b.wo.z <= 0 ||
             fabsf(dot(frame_reflect(b.wi), b.wo) - 1) > DeltaEpsilon);
}
inline Spec conductor_f(const ctl_material& m, const ctl_material_ext& e, const BRec& b, int measure) {
    if (!conductor_pair(b, measure)) return v3s(0.0f);
    return c5::spec_refl(m) * fresnel_conductor_exact(b.wi.z, ext_eta(e), ext_k(e));
}
inline float conductor_pdf(const BRec& b, int measure) { return conductor_pair(b, measure) ? 1.0f : 0.0f; }

// ---------------------------------------------------------------- roughconductor
// m_sampleVisible only (MicrofacetDistribution::sample's visible branch,
// MicrofacetDistribution.h:71-77); the dispatch refuses the other.
inline Spec roughconductor_sample(const ctl_material& m, const ctl_material_ext& e, BRec& b, float& pdf, V2 sample) {
    if (b.wi.z < 0 || !(b.typeMask & CTL_EGLOSSY_REFLECTION)) return v3s(0.0f);
    c5::Distr distr = c5::distr_of(m);
    const V3 mm = c5::d_sample_visible(distr, b.wi, sample);
    pdf = c5::d_pdf_visible(distr, b.wi, mm);
    if (pdf == 0) return v3s(0.0f);
    b.wo = c5::reflect(b.wi, mm);
    b.sampledType = CTL_EGLOSSY_REFLECTION;
    if (b.wo.z <= 0) return v3s(0.0f);
    const Spec F = fresnel_conductor_exact(dot(b.wi, mm), ext_eta(e), ext_k(e)) * c5::spec_refl(m);
    float weight = c5::d_G1(distr, b.wo, mm);
    pdf /= 4.0f * dot(b.wo, mm);
    return F * weight;
}
inline Spec roughconductor_f(const ctl_material& m, const ctl_material_ext& e, const BRec& b, int measure) {
    if (measure != MSolidAngle || b.wi.z < 0 || b.wo.z < 0 || !(b.typeMask & CTL_EGLOSSY_REFLECTION)) return v3s(0.0f);
    V3 H = normalize(b.wo + b.wi);
    c5::Distr distr = c5::distr_of(m);
    const float D = c5::d_eval(distr, H);
    if (D == 0) return v3s(0.0f);
    const Spec F = fresnel_conductor_exact(dot(b.wi, H), ext_eta(e), ext_k(e)) * c5::spec_refl(m);
    const float G = c5::d_G(distr, b.wi, b.wo, H);
    float value = D * G / (4.0f * b.wi.z);
    return F * value;
}
inline float roughconductor_pdf(const ctl_material& m, const BRec& b, int measure) {
    if (measure != MSolidAngle || b.wi.z < 0 || b.wo.z < 0 || !(b.typeMask & CTL_EGLOSSY_REFLECTION)) return 0.0f;
    V3 H = normalize(b.wo + b.wi);
    c5::Distr distr = c5::distr_of(m);
    return c5::d_eval(distr, H) * c5::d_G1(distr, b.wi, H) / (4.0f * b.wi.z);
}

// ---------------------------------------------------------------- plastic
inline float plastic_prob_specular(const ctl_material_ext& e, float Fi) {
    return (Fi * e.specular_sampling_weight) /
           (Fi * e.specular_sampling_weight + (1 - Fi) * (1 - e.specular_sampling_weight));
}
// m_diffuseReflectance.Evaluate(dg), then the internal-scattering denominator (BSDF_Simple.cu:797-801)
inline Spec plastic_diff(const ctl_scene_desc* d, const ctl_material& m, const ctl_material_ext& e, const DG& dg) {
    Spec diff = diffuse_R(d, m, dg);
    if (e.nonlinear) return sdiv(diff, v3s(1.0f) - diff * e.fdr_int);
    return spec_div(diff, 1 - e.fdr_int);
}

inline Spec plastic_sample(const ctl_scene_desc* d, const ctl_material& m, const ctl_material_ext& e, BRec& b, float& pdf,
                           V2 sample) {
    bool hasSpecular = (b.typeMask & CTL_EDELTA_REFLECTION) != 0;
    bool hasDiffuse = (b.typeMask & CTL_EDIFFUSE_REFLECTION) != 0;
    if ((!hasDiffuse && !hasSpecular) || b.wi.z <= 0) return v3s(0.0f);
    float Fi = c5::fresnel_ext(b.wi.z, m.eta);
    if (hasDiffuse && hasSpecular) {
        float probSpecular = plastic_prob_specular(e, Fi);
        if (sample.x < probSpecular) {
            b.sampledType = CTL_EDELTA_REFLECTION;
            b.wo = frame_reflect(b.wi);
            pdf = probSpecular;
            return spec_div(ext_specular(e) * Fi, probSpecular);
        } else {
            b.sampledType = CTL_EDIFFUSE_REFLECTION;
            b.wo = cosine_hemisphere(v2((sample.x - probSpecular) / (1 - probSpecular), sample.y));
            float Fo = c5::fresnel_ext(b.wo.z, m.eta);
            Spec diff = plastic_diff(d, m, e, b.dg);
            pdf = (1 - probSpecular) * cosine_hemisphere_pdf(b.wo);
            return diff * (e.inv_eta2 * (1 - Fi) * (1 - Fo) / (1 - probSpecular));
        }
    } else if (hasSpecular) {
        b.sampledType = CTL_EDELTA_REFLECTION;
        b.wo = frame_reflect(b.wi);
        pdf = 1;
        return ext_specular(e) * Fi;
    } else {
        b.sampledType = CTL_EDIFFUSE_REFLECTION;
        b.wo = cosine_hemisphere(sample);
        float Fo = c5::fresnel_ext(b.wo.z, m.eta);
        Spec diff = plastic_diff(d, m, e, b.dg);
        pdf = cosine_hemisphere_pdf(b.wo);
        return diff * (e.inv_eta2 * (1 - Fi) * (1 - Fo));
    }
}

inline Spec plastic_f(const ctl_scene_desc* d, const ctl_material& m, const ctl_material_ext& e, const BRec& b,
                      int measure) {
    bool hasSpecular = (b.typeMask & CTL_EDELTA_REFLECTION) && measure == MDiscrete;
    bool hasDiffuse = (b.typeMask & CTL_EDIFFUSE_REFLECTION) && measure == MSolidAngle;
    if (b.wo.z <= 0 || b.wi.z <= 0) return v3s(0.0f);
    float Fi = c5::fresnel_ext(b.wi.z, m.eta);
    if (hasSpecular) {
        if (fabsf(dot(frame_reflect(b.wi), b.wo) - 1) < DeltaEpsilon) return ext_specular(e) * Fi;
    } else if (hasDiffuse) {
        float Fo = c5::fresnel_ext(b.wo.z, m.eta);
        Spec diff = plastic_diff(d, m, e, b.dg);
        return diff * (cosine_hemisphere_pdf(b.wo) * e.inv_eta2 * (1 - Fi) * (1 - Fo));
    }
    return v3s(0.0f);
}

inline float plastic_pdf(const ctl_material& m, const ctl_material_ext& e, const BRec& b, int measure) {
    bool hasSpecular = (b.typeMask & CTL_EDELTA_REFLECTION) != 0;
    bool hasDiffuse = (b.typeMask & CTL_EDIFFUSE_REFLECTION) != 0;
    if (b.wo.z <= 0 || b.wi.z <= 0) return 0.0f;
    float probSpecular = hasSpecular ? 1.0f : 0.0f;
    if (hasSpecular && hasDiffuse) {
        float Fi = c5::fresnel_ext(b.wi.z, m.eta);
        probSpecular = plastic_prob_specular(e, Fi);
    }
    if (hasSpecular && measure == MDiscrete) {
        if (fabsf(dot(frame_reflect(b.wi), b.wo) - 1) < DeltaEpsilon) return probSpecular;
    } else if (hasDiffuse && measure == MSolidAngle) {
        return cosine_hemisphere_pdf(b.wo) * (1 - probSpecular);
    }
    return 0.0f;
}

}  // namespace omat
