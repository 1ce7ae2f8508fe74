// medium_eval.hip — the batch medium entry: the five operations of
// csrc/ctl_medium.h (IntersectP, Transmittance, sampleDistance, the aggregate's p
// and Sample; SceneTypes/Volumes.cu, Kernel/TraceAlgorithms.cu:22-31) for an
// array of queries against a scene's volume, on the device (ctl_medium_eval, the
// uploaded scene) and on the host (ctl_host_medium_eval, a scene description).
// Both run eval_query below.
#include <hip/hip_runtime.h>

#include <string>

#include "../../../include/ctl_trace.h"
#include "common.h"

using namespace ctl;

static_assert(sizeof(ctl_medium_result) == 96 && sizeof(ctl_medium_query) == 56, "medium records");

namespace {

CTL_HD void put3(float* o, f3 v) { o[0] = v.x; o[1] = v.y; o[2] = v.z; }

// Every field an op does not write is 0; no volume or an unknown op: all 0.
CTL_HD ctl_medium_result eval_query(const ctl_volume* vol, const ctl_medium_query& q) {
    ctl_medium_result r;
    r.hit = 0;
    r.t0 = r.t1 = r.t = 0.0f;
    r.pdf_success = r.pdf_success_rev = r.pdf_failure = r.value = r.pdf = 0.0f;
    for (int k = 0; k < 3; k++) r.p[k] = r.transmittance[k] = r.sigma_a[k] = r.sigma_s[k] = r.wo_out[k] = 0.0f;
    if (!vol) return r;
    const ctl_volume& V = *vol;
    const f3 ori = mk3(q.ori[0], q.ori[1], q.ori[2]), dir = mk3(q.dir[0], q.dir[1], q.dir[2]);
    switch (q.op) {
        case CTL_MEDIUM_INTERSECT: {
            float t0 = 0.0f, t1 = 0.0f;
            r.hit = medium_intersect(V, ori, dir, q.tmin, q.tmax, t0, t1) ? 1u : 0u;
            r.t0 = t0; r.t1 = t1;
            break;
        }
        case CTL_MEDIUM_TRANSMITTANCE: {
            float t0 = 0.0f, t1 = 0.0f;
            r.hit = medium_intersect(V, ori, dir, q.tmin, q.tmax, t0, t1) ? 1u : 0u;
            r.t0 = t0; r.t1 = t1;
            put3(r.transmittance, medium_transmittance(V, ori, dir, q.tmin, q.tmax));
            break;
        }
        case CTL_MEDIUM_SAMPLE_DISTANCE: {
            medium_rec m;
            m.t = 0.0f;
            m.p = m.sigmaA = m.sigmaS = mk3s(0.0f);
            r.hit = medium_sample_distance(V, ori, dir, q.tmin, q.tmax, q.u[0], m) ? 1u : 0u;
            r.t = m.t;
            put3(r.p, m.p);
            put3(r.transmittance, m.transmittance);
            put3(r.sigma_a, m.sigmaA);
            put3(r.sigma_s, m.sigmaS);
            r.pdf_success = m.pdfSuccess;
            r.pdf_success_rev = m.pdfSuccessRev;
            r.pdf_failure = m.pdfFailure;
            break;
        }
        case CTL_MEDIUM_PHASE_EVAL:
            r.value = medium_phase_eval(V, ori, dir, mk3(q.wo[0], q.wo[1], q.wo[2]));
            break;
        case CTL_MEDIUM_PHASE_SAMPLE: {
            f3 wo = mk3s(0.0f);
            float w = 0.0f, pdf = 0.0f;
            r.hit = medium_phase_sample(V, ori, dir, mk2(q.u[0], q.u[1]), wo, w, pdf) ? 1u : 0u;
            put3(r.wo_out, wo);
            r.value = w;
            r.pdf = pdf;
            break;
        }
        default: break;
    }
    // a NaN's sign and payload are the host's or the device's choice (which operand a
    // division passes on): every NaN leaves as the same one, as in light_eval.hip
    float* f = &r.t0;
    for (int k = 0; k < 23; k++)
        if (f[k] != f[k]) f[k] = bits_f(0x7fc00000);
    return r;
}

// The record is the same for every lane: it is read through the kernel argument,
// a uniform address.
__global__ __launch_bounds__(kBlock) void medium_eval_kernel(const ctl_volume* vol, uint64_t n, const ctl_medium_query* q,
                                                             ctl_medium_result* out) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    out[i] = eval_query(vol, q[i]);
}

}  // namespace

namespace ctl {
void set_host_error(const std::string& s);   // host/scene.cpp
}

extern "C" {

CTL_API ctl_status ctl_medium_eval(ctl_ctx* c, const ctl_medium_query* d_queries, int64_t n, ctl_medium_result* d_results,
                                   void* stream) {
    if (!c) return CTL_ERR_INVALID;
    if (!c->has_scene) { c->err = "medium_eval: no scene uploaded"; return CTL_ERR_STATE; }
    if (n < 0) { c->err = "medium_eval: negative query count"; return CTL_ERR_INVALID; }
    if (n == 0) return CTL_OK;
    if (!d_queries || !d_results) { c->err = "medium_eval: null query or result array"; return CTL_ERR_INVALID; }
    const uint64_t blocks = ((uint64_t)n + kBlock - 1) / kBlock;
    if (blocks > 0x7fffffffull) { c->err = "medium_eval: too many queries for one launch"; return CTL_ERR_INVALID; }
    if (hipSetDevice(c->device) != hipSuccess) { c->err = "medium_eval: hipSetDevice failed"; return CTL_ERR_HIP; }
    hipLaunchKernelGGL(medium_eval_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream),
                       c->d_volume, (uint64_t)n, d_queries, d_results);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { c->err = std::string("medium_eval: ") + hipGetErrorString(e); return CTL_ERR_HIP; }
    return CTL_OK;
}

CTL_API ctl_status ctl_host_medium_eval(const ctl_scene_desc* d, const ctl_medium_query* queries, int64_t n,
                                        ctl_medium_result* results) {
    if (!d || n < 0 || (n && (!queries || !results))) { set_host_error("host_medium_eval: invalid argument"); return CTL_ERR_INVALID; }
    if (d->n_volumes > 1) { set_host_error("host_medium_eval: more than one volume"); return CTL_ERR_INVALID; }
    if (d->n_volumes && !d->volumes) { set_host_error("host_medium_eval: n_volumes without the record"); return CTL_ERR_INVALID; }
    if (d->n_volumes)
        if (const char* why = volume_check(d->volumes[0])) { set_host_error(std::string("host_medium_eval: ") + why); return CTL_ERR_INVALID; }
    const ctl_volume* vol = d->n_volumes ? d->volumes : nullptr;
    for (int64_t i = 0; i < n; i++) results[i] = eval_query(vol, queries[i]);
    return CTL_OK;
}

}  // extern "C"
