// light_eval.hip — the batch light entry: Light::sampleDirect
// (SceneTypes/Light.h:34-292, Light.cu) for an array of queries against a
// scene's lights, on the device (ctl_light_eval, the uploaded scene) and on the
// host (ctl_host_light_eval, a scene description).  Both run eval_query below,
// which calls light_sample_direct_any of ctl_light.h, the dispatch the
// integrators' light sample goes through (sample_light_direct, shading.h), in
// its five-kind form.
#include <hip/hip_runtime.h>

#include <string>

#include "../../../include/ctl_trace.h"
#include "common.h"

using namespace ctl;

namespace {

struct LightScene {
    const ctl_light* lights;
    uint32_t n_lights;
    const ctl_light_tri* tris;
    const float* cdfs;
    EnvView env;
};

// A query naming a light the scene does not have: zero value, measure all ones.
// The record starts as DirectSamplingRecord(ref, refN) does in the integrators (nee_sample), with pdf 0.
CTL_HD ctl_light_result eval_query(const LightScene& S, const ctl_light_query& q) {
    ctl_light_result r;
    for (int k = 0; k < 3; k++) r.value[k] = r.d[k] = r.p[k] = r.n[k] = 0.0f;
    r.pdf = r.dist = 0.0f;
    r.measure = 0xffffffffu;
    r.pad = 0;
    if (q.light >= S.n_lights) return r;
    direct_rec dRec;
    dRec.ref = mk3(q.ref[0], q.ref[1], q.ref[2]);
    dRec.refN = mk3(q.ref_n[0], q.ref_n[1], q.ref_n[2]);
    dRec.p = dRec.ref; dRec.n = dRec.refN;
    dRec.d = mk3s(0.0f);
    dRec.dist = 0.0f; dRec.pdf = 0.0f;
    dRec.measure = kEArea;
    const spec v = light_sample_direct_any<true, true>(S.lights, S.tris, S.cdfs, S.env, q.light, dRec,
                                                       mk2(q.sample[0], q.sample[1]));
    r.value[0] = v.x; r.value[1] = v.y; r.value[2] = v.z;
    r.pdf = dRec.pdf;
    r.d[0] = dRec.d.x; r.d[1] = dRec.d.y; r.d[2] = dRec.d.z;
    r.dist = dRec.dist;
    r.p[0] = dRec.p.x; r.p[1] = dRec.p.y; r.p[2] = dRec.p.z;
    r.measure = (uint32_t)dRec.measure;
    r.n[0] = dRec.n.x; r.n[1] = dRec.n.y; r.n[2] = dRec.n.z;
    return r;
}

__global__ __launch_bounds__(kBlock) void light_eval_kernel(LightScene S, uint64_t n, const ctl_light_query* q,
                                                            ctl_light_result* out) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    out[i] = eval_query(S, q[i]);
}

// The light checks of ctl_scene_upload that keep eval_query's reads in bounds,
// for a description that was never uploaded.
bool host_lights_ok(const ctl_scene_desc* d, std::string& err) {
    if (d->n_lights > CTL_MAX_NUM_LIGHTS) { err = "host_light_eval: more than 16 lights"; return false; }
    for (uint32_t i = 0; i < d->n_lights; i++) {
        const ctl_light& L = d->lights[i];
        const std::string who = "host_light_eval: light " + std::to_string(i) + ": ";
        if (L.kind > CTL_LIGHT_DISTANT) { err = who + "unknown kind"; return false; }
        if (L.kind == CTL_LIGHT_DIFFUSE) {
            if (L.tri_count == 0 || (uint64_t)L.tri_first + L.tri_count > d->n_light_tris ||
                (uint64_t)L.cdf_first + L.tri_count + 1 > d->n_light_tri_cdf) {
                err = who + "triangles or CDF outside the scene's arrays";
                return false;
            }
        } else if (L.kind == CTL_LIGHT_INFINITE) {
            const ctl_env_light* e = d->env;
            if (i != d->env_map_index || !e || e->texture >= d->n_textures || !d->env_data) {
                err = who + "environment light without its record, texture or tables";
                return false;
            }
            const uint64_t w = d->textures[e->texture].width, h = d->textures[e->texture].height;
            if ((uint64_t)e->cdf_cols + (w + 1) * h > d->n_env_data || (uint64_t)e->cdf_rows + h + 1 > d->n_env_data ||
                (uint64_t)e->row_weights + h > d->n_env_data) {
                err = who + "environment tables do not match the radiance map";
                return false;
            }
        } else if (const char* why = delta_light_check(L, d->light_tris, d->n_light_tris)) {
            err = who + why;
            return false;
        }
    }
    return true;
}

}  // namespace

namespace ctl {
void set_host_error(const std::string& s);   // host/scene.cpp
}

extern "C" {

CTL_API ctl_status ctl_light_eval(ctl_ctx* c, const ctl_light_query* d_queries, int64_t n, ctl_light_result* d_results,
                                  void* stream) {
    if (!c) return CTL_ERR_INVALID;
    if (!c->has_scene) { c->err = "light_eval: no scene uploaded"; return CTL_ERR_STATE; }
    if (n < 0) { c->err = "light_eval: negative query count"; return CTL_ERR_INVALID; }
    if (n == 0) return CTL_OK;
    if (!d_queries || !d_results) { c->err = "light_eval: null query or result array"; return CTL_ERR_INVALID; }
    const uint64_t blocks = ((uint64_t)n + kBlock - 1) / kBlock;
    if (blocks > 0x7fffffffull) { c->err = "light_eval: too many queries for one launch"; return CTL_ERR_INVALID; }
    if (hipSetDevice(c->device) != hipSuccess) { c->err = "light_eval: hipSetDevice failed"; return CTL_ERR_HIP; }
    const DevScene& S = c->scene;
    const LightScene LS{S.lights, S.n_lights, S.light_tris, S.light_tri_cdf, EnvView{S.env, S.env_data, S.textures, S.tex_data}};
    hipLaunchKernelGGL(light_eval_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream),
                       LS, (uint64_t)n, d_queries, d_results);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { c->err = std::string("light_eval: ") + hipGetErrorString(e); return CTL_ERR_HIP; }
    return CTL_OK;
}

CTL_API ctl_status ctl_host_light_eval(const ctl_scene_desc* d, const ctl_light_query* queries, int64_t n,
                                       ctl_light_result* results) {
    if (!d || n < 0 || (n && (!queries || !results))) { set_host_error("host_light_eval: invalid argument"); return CTL_ERR_INVALID; }
    std::string err;
    if (!host_lights_ok(d, err)) { set_host_error(err); return CTL_ERR_INVALID; }
    const LightScene LS{d->lights, d->n_lights, d->light_tris, d->light_tri_cdf,
                        EnvView{d->env, d->env_data, d->textures, d->tex_data}};
    for (int64_t i = 0; i < n; i++) results[i] = eval_query(LS, queries[i]);
    return CTL_OK;
}

}  // extern "C"
