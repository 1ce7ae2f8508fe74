// math_eval.hip — the batch entry for the scalar arithmetic: the cr_*
// transcendentals of ctl_math.h, erf_ref / erfinv_ref of ctl_bsdf.h, fp32
// division, sqrtf, rcp_ref and the 16-bit helpers, for arrays of inputs, on
// the device (ctl_math_eval) and on the host (ctl_host_math_eval).  Both run
// eval_one below, which calls the functions of the headers that the kernels
// and the host scene compiler call (on the device the out-of-line CTL_CR
// bodies), so a difference between the two entries is a difference between
// the device's and the host's arithmetic.  No scene is needed.
#include <hip/hip_runtime.h>

#include <string>

#include "../../../include/ctl_trace.h"
#include "common.h"

using namespace ctl;

namespace {

// Element i of function fn (the CTL_MATH_* table of ctl_trace.h).
CTL_HD void eval_one(uint32_t fn, uint64_t i, const float* a, const float* b, uint32_t* out) {
    const float x = (fn == CTL_MATH_NORMAL_ENCODE16) ? 0.0f : a[i];
    const uint32_t u = (uint32_t)f_bits(x);   // the decodes' integer input
    float r = 0.0f;
    switch (fn) {
        case CTL_MATH_SIN: r = cr_sin(x); break;
        case CTL_MATH_COS: r = cr_cos(x); break;
        case CTL_MATH_TAN: r = cr_tan(x); break;
        case CTL_MATH_ACOS: r = cr_acos(x); break;
        case CTL_MATH_ATAN: r = cr_atan(x); break;
        case CTL_MATH_ATAN2: r = cr_atan2(x, b[i]); break;
        case CTL_MATH_EXP: r = cr_exp(x); break;
        case CTL_MATH_LOG: r = cr_log(x); break;
        case CTL_MATH_LOG2: r = cr_log2(x); break;
        case CTL_MATH_POW: r = cr_pow(x, b[i]); break;
        case CTL_MATH_ERF: r = erf_ref(x); break;
        case CTL_MATH_ERFINV: r = erfinv_ref(x); break;
        case CTL_MATH_DIV: r = x / b[i]; break;
        case CTL_MATH_SQRT: r = sqrtf(x); break;
        case CTL_MATH_RCP: r = rcp_ref(x); break;
        case CTL_MATH_HALF_IEEE: r = half_to_float(u, false); break;
        case CTL_MATH_HALF_QUIRK: r = half_to_float(u, true); break;
        case CTL_MATH_HALF_ROUND_INT: r = half_round_int(u); break;
        case CTL_MATH_U16_TRUNC: out[i] = (uint32_t)u16_trunc(x); return;
        case CTL_MATH_NORMAL_ENCODE16:
            out[i] = (uint32_t)normal_encode16(mk3(a[3 * i], a[3 * i + 1], a[3 * i + 2]));
            return;
        case CTL_MATH_NORMAL_DECODE16: {
            const f3 v = normal_decode16(u);
            out[3 * i] = (uint32_t)f_bits(v.x); out[3 * i + 1] = (uint32_t)f_bits(v.y); out[3 * i + 2] = (uint32_t)f_bits(v.z);
            return;
        }
        default: break;
    }
    out[i] = (uint32_t)f_bits(r);
}

bool two_arguments(uint32_t fn) { return fn == CTL_MATH_ATAN2 || fn == CTL_MATH_POW || fn == CTL_MATH_DIV; }

__global__ __launch_bounds__(kBlock) void math_eval_kernel(uint32_t fn, uint64_t n, const float* a, const float* b,
                                                           uint32_t* out) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    eval_one(fn, i, a, b, out);
}

}  // namespace

namespace ctl {
void set_host_error(const std::string& s);   // host/scene.cpp
}

extern "C" {

CTL_API ctl_status ctl_math_eval(ctl_ctx* c, uint32_t fn, uint64_t n, const float* d_a, const float* d_b, uint32_t* d_out,
                                 void* stream) {
    if (!c) return CTL_ERR_INVALID;
    if (fn >= CTL_MATH_COUNT) { c->err = "math_eval: unknown function id"; return CTL_ERR_INVALID; }
    if (n == 0) return CTL_OK;
    if (!d_a || !d_out || (two_arguments(fn) && !d_b)) { c->err = "math_eval: null input or output array"; return CTL_ERR_INVALID; }
    const uint64_t blocks = (n + kBlock - 1) / kBlock;
    if (blocks > 0x7fffffffull) { c->err = "math_eval: too many elements for one launch"; return CTL_ERR_INVALID; }
    if (hipSetDevice(c->device) != hipSuccess) { c->err = "math_eval: hipSetDevice failed"; return CTL_ERR_HIP; }
    hipLaunchKernelGGL(math_eval_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream), fn, n,
                       d_a, d_b, d_out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { c->err = std::string("math_eval: ") + hipGetErrorString(e); return CTL_ERR_HIP; }
    return CTL_OK;
}

CTL_API ctl_status ctl_host_math_eval(uint32_t fn, uint64_t n, const float* a, const float* b, uint32_t* out) {
    if (fn >= CTL_MATH_COUNT) { set_host_error("host_math_eval: unknown function id"); return CTL_ERR_INVALID; }
    if (n && (!a || !out || (two_arguments(fn) && !b))) { set_host_error("host_math_eval: null argument"); return CTL_ERR_INVALID; }
    for (uint64_t i = 0; i < n; i++)
        eval_one(fn, i, a, b, out);
    return CTL_OK;
}

}  // extern "C"
