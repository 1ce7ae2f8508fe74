// ctl_image.h — fp32 arithmetic of the final-image stage, shared by the gfx950
// kernels (device/image.hip, device/pipeline.hip) and the host helpers of the
// C ABI (ctl_filter_evaluate, ctl_rgbe_encode, ...).  Reference operation order
// throughout (the library is built with -ffp-contract=off); transcendentals go
// through the correctly-rounded cr_* of ctl_math.h.
#pragma once
#include "ctl_shade.h"

namespace ctl {

// ---- sRGB / RGBCOL ---------------------------------------------------------

// toSRGBComponent (Math/Spectrum.cu:229-234)
CTL_HD float to_srgb(float v) {
    if (v <= (float)0.0031308) return (float)12.92 * v;
    return (float)1.055 * cr_pow(v, (float)(1.0 / 2.4)) - (float)0.055;
}
// SpectrumConverter::Float3ToCOLORREF (Math/Spectrum.h:521-526); NaN -> 0 (clamp01's max picks 0)
CTL_HD uint32_t to_u8(float x) { return (uint32_t)(unsigned char)(tmin(tmax(x, 0.0f), 1.0f) * 255.0f); }
// Spectrum::toRGBCOL (Math/Spectrum.cu:273-278): r in the low byte, a = 255
CTL_HD uint32_t to_rgbcol(spec c) { return to_u8(c.x) | (to_u8(c.y) << 8) | (to_u8(c.z) << 16) | (255u << 24); }
// SpectrumConverter::COLORREFToFloat3 (Math/Spectrum.h:528-532)
CTL_HD spec from_rgbcol(uint32_t c) {
    return mk3(float(c & 0xffu) / 255.0f, float((c >> 8) & 0xffu) / 255.0f, float((c >> 16) & 0xffu) / 255.0f);
}
// gammaCorrecture (Kernel/ImagePipeline/ImagePipeline.cu:7-12)
CTL_HD uint32_t gamma_correct(spec c) { return to_rgbcol(mk3(to_srgb(c.x), to_srgb(c.y), to_srgb(c.z))); }

// PixelData::toSpectrum (Engine/Image.h:21-28)
CTL_HD spec pixel_to_spectrum(const ctl_pixel& p, float splat) {
    const float weight = p.weight_sum != 0 ? p.weight_sum : 1;
    return spec_div(mk3(p.rgb[0], p.rgb[1], p.rgb[2]), weight) + mk3(p.rgb_splat[0], p.rgb_splat[1], p.rgb_splat[2]) * splat;
}

// ---- RGBE (one uint32, little-endian r, g, b, e) ---------------------------

// (unsigned char)(c * max_) made total: truncate, saturate to 0..255, NaN -> 0
// (the reference's conversion is undefined outside 0..255).
CTL_HD uint32_t rgbe_byte(float v) {
    if (!(v > 0.0f)) return 0u;
    if (v >= 255.0f) return 255u;
    return (uint32_t)(int32_t)v;
}
// SpectrumConverter::Float3ToRGBE (Math/Spectrum.h:534-555).  frexp_self
// (Spectrum.h:480-513) of the widened float: its fraction is the float's own
// mantissa with exponent -1, so it is taken from the float's bits.  An infinite
// or NaN maximum leaves the reference's exponent uninitialised; here e = 0.
CTL_HD uint32_t rgbe_encode(spec c) {
    float max_ = tmax(tmax(c.x, c.y), c.z);   // max(a, b, c) = max(max(a, b), c), MathFunc.h:93
    if ((double)max_ < 1e-32) return 0u;
    const uint32_t b = (uint32_t)f_bits(max_);
    int e = 0;
    float frac = max_;
    if (((b >> 23) & 0xffu) != 0xffu) {
        e = (int)((b >> 23) & 0xffu) - 126;
        frac = bits_f((int32_t)((b & 0x807fffffu) | (126u << 23)));
    }
    max_ = frac * 256.0f / max_;
    return rgbe_byte(c.x * max_) | (rgbe_byte(c.y * max_) << 8) | (rgbe_byte(c.z * max_) << 16) |
           ((uint32_t)((e + 128) & 0xff) << 24);
}
// SpectrumConverter::RGBEToFloat3 (Math/Spectrum.h:557-565); ldexp(1.0f, e - 136) from its bits
CTL_HD spec rgbe_decode(uint32_t v) {
    const int w = (int)(v >> 24);
    if (!w) return mk3s(0.0f);
    const int ex = w - (128 + 8);   // -135 .. 119
    const float exp = ex >= -126 ? bits_f((int32_t)((uint32_t)(ex + 127) << 23)) : bits_f((int32_t)(1u << (149 + ex)));
    return mk3(float(v & 0xffu) * exp, float((v >> 8) & 0xffu) * exp, float((v >> 16) & 0xffu) * exp);
}

// ---- colour spaces (Math/Spectrum.cu, the RGB build) -----------------------

CTL_HD float clamp_ref(float v, float lo, float hi) { return tmin(tmax(v, lo), hi); }   // MathFunc.h:170
// Spectrum::toXYZ (Spectrum.cu:160-165)
CTL_HD void to_xyz(spec s, float& x, float& y, float& z) {
    x = s.x * 0.412453f + s.y * 0.357580f + s.z * 0.180423f;
    y = s.x * 0.212671f + s.y * 0.715160f + s.z * 0.072169f;
    z = s.x * 0.019334f + s.y * 0.119193f + s.z * 0.950227f;
}
// Spectrum::fromXYZ (Spectrum.cu:167-172)
CTL_HD spec from_xyz(float x, float y, float z) {
    return mk3(3.240479f * x + -1.537150f * y + -0.498535f * z, -0.969256f * x + 1.875991f * y + 0.041556f * z,
               0.055648f * x + -0.204043f * y + 1.057311f * z);
}
// Spectrum::getLuminance (Spectrum.cu:174-177)
CTL_HD float get_luminance(spec s) { return s.x * 0.212671f + s.y * 0.715160f + s.z * 0.072169f; }
// Spectrum::toYxy (Spectrum.cu:286-294)
CTL_HD void to_Yxy(spec c, float& _Y, float& x, float& y) {
    float X, Y, Z;
    to_xyz(c, X, Y, Z);
    const float s = clamp_ref(X + Y + Z, 0.001f, 100000.0f);
    _Y = Y;
    x = X / s;
    y = Y / s;
}
// Spectrum::fromYxy (Spectrum.cu:296-302)
CTL_HD spec from_Yxy(float _Y, float x, float y) {
    const float X = _Y / clamp_ref(y, 0.001f, 100000.0f) * x;
    const float Y = _Y;
    const float Z = _Y / clamp_ref(y, 0.001f, 100000.0f) * (1 - x - y);
    return from_xyz(X, Y, Z);
}

// ---- Reinhard tone map (PostProcess/ToneMapPostProcess.cu) -----------------

// ToneMapPostProcess::Apply's constants (ToneMapPostProcess.cu:26-38)
CTL_HD void tonemap_constants(float key, float burn_in, float avg_log_lum, float max_lum, float& scale, float& inv_wp2) {
    scale = key / avg_log_lum;
    const float Lwhite = max_lum * scale;
    const float burn = tmin(1.0f, tmax(1e-8f, 1.0f - burn_in));
    inv_wp2 = 1 / (Lwhite * Lwhite * cr_pow(burn, 4.0f));
}
// Reinhard05Kernel's pixel (ToneMapPostProcess.cu:6-24): linear RGBCOL
CTL_HD uint32_t reinhard_pixel(uint32_t rgbe, float scale, float inv_wp2) {
    const spec color = rgbe_decode(rgbe);
    float x, y, Y;
    to_Yxy(color, Y, x, y);
    const float Lp = scale * Y;
    Y = Lp * (1.0f + Lp * inv_wp2) / (1.0f + Lp);
    return to_rgbcol(from_Yxy(Y, x, y));
}

// ---- reconstruction filters (SceneTypes/Filter.h:28-171) -------------------

// Every canonical Filter::Evaluate(x, y) is a product of one factor per axis
// (the box filter's is 1); filter_factor is that factor for axis 0 (x) or 1 (y).
CTL_HD float mitchell_1d(float B, float C, float x) {   // MitchellFilter::Mitchell1D (Filter.h:96-106)
    x = fabsf(2.f * x);
    if (x > 1.f)
        return ((-B - 6 * C) * x * x * x + (6 * B + 30 * C) * x * x + (-12 * B - 48 * C) * x + (8 * B + 24 * C)) *
               (1.f / 6.f);
    else
        return ((12 - 9 * B - 6 * C) * x * x * x + (-18 + 12 * B + 6 * C) * x * x + (6 - 2 * B)) * (1.f / 6.f);
}
CTL_HD float lanczos_sinc_1d(float tau, float x) {      // LanczosSincFilter::Sinc1D (Filter.h:131-139)
    x = fabsf(x);
    if ((double)x < 1e-5) return 1.f;
    if ((double)x > 1.) return 0.f;
    x *= CTL_PI;
    const float sinc = cr_sin(x) / x;
    const float lanczos = cr_sin(x * tau) / (x * tau);
    return sinc * lanczos;
}
CTL_HD float filter_factor(const ctl_image_filter& f, float d, int axis) {
    const float width = axis ? f.y_width : f.x_width;
    switch (f.type) {
    case CTL_FILTER_GAUSSIAN: {   // GaussianFilter::Update + Gaussian (Filter.h:66-75)
        const float alpha = f.a;
        const float expv = cr_exp(-alpha * width * width);
        return tmax(0.f, float(cr_exp(-alpha * d * d) - expv));
    }
    case CTL_FILTER_MITCHELL: return mitchell_1d(f.a, f.b, d * (1.0f / width));       // Filter.h:108-111, FilterBase::Update :20-24
    case CTL_FILTER_LANCZOS: return lanczos_sinc_1d(f.a, d * (1.0f / width));         // Filter.h:141-144
    case CTL_FILTER_TRIANGLE: return tmax(0.f, width - fabsf(d));                     // Filter.h:166-169
    default: return 1.0f;                                                             // BoxFilter (Filter.h:43-46)
    }
}
CTL_HD float filter_evaluate(const ctl_image_filter& f, float x, float y) {
    if (f.type == CTL_FILTER_BOX) return 1;
    return filter_factor(f, x, 0) * filter_factor(f, y, 1);
}

// ---- variance-guided non-local means (Filter/NonLocalMeansFilter.cu) -------

// half(float) on the reference's device path: __float2half_rn (Math/half.h:21-25),
// IEEE binary16, round to nearest even.
CTL_HD uint32_t float_to_half_rn(float f) {
    const uint32_t b = (uint32_t)f_bits(f), sign = (b >> 16) & 0x8000u, a = b & 0x7fffffffu;
    if (a > 0x7f800000u) return sign | 0x7fffu;      // NaN
    if (a >= 0x477ff000u) return sign | 0x7c00u;     // >= 65520 rounds to infinity
    if (a <= 0x33000000u) return sign;               // <= 2^-25 rounds to zero (the tie goes to even)
    const int e = (int)(a >> 23) - 127;
    const uint32_t m = (a & 0x7fffffu) | 0x800000u;
    const uint32_t shift = e < -14 ? (uint32_t)(13 + (-14 - e)) : 13u;   // 13 .. 24 bits dropped
    uint32_t q = m >> shift;
    const uint32_t r = m & ((1u << shift) - 1u), h = 1u << (shift - 1u);
    if (r > h || (r == h && (q & 1u))) q++;
    return sign | (e < -14 ? q : (uint32_t)((e + 14) << 10) + q);   // q carries the implicit bit into the exponent
}
// PixelVarianceInfo::computeVariance (PixelVarianceBuffer.h:53-57) stored as half
// and read back (copyToShared / loadFromShared, NonLocalMeansFilter.cu:32,52),
// times sigma2Scale (:83)
CTL_HD float nlm_variance(const ctl_pixel_variance& v, float sigma2_scale) {
    const float N = (float)v.num_samples_var;
    const float invN = 1.0f / N;
    const float variance = (v.sum_x2 - (v.sum_x * v.sum_x) * invN) * invN;
    return half_to_float(float_to_half_rn(variance), false) * sigma2_scale;
}
// One tap of patchDistance (NonLocalMeansFilter.cu:81-86); the variances are already scaled
CTL_HD float nlm_tap(spec c_p, spec c_q, float var_p, float var_q, float k) {
    const float eps = 1e-10f;
    const spec df = c_p - c_q;
    const spec sq = df * df;
    float sum = 0.0f; sum += sq.x; sum += sq.y; sum += sq.z;   // TSpectrum::sum / avg (Spectrum.h:180-189)
    const float u_diff = sum * (1.0f / 3);
    return (u_diff - (var_p + tmin(var_p, var_q))) / (eps + k * k * (var_p + var_q));
}
// patchDistance's mean and weight (NonLocalMeansFilter.cu:91-99); fmaxf: a NaN distance weighs 1
CTL_HD float nlm_weight(float d_sum, float taps) {
    const float d_range = taps != 0 ? d_sum / taps : 0;
    const float w = cr_exp(-fmaxf(0.0f, d_range));
    return w < 0.05f ? 0.0f : w;
}

}  // namespace ctl
