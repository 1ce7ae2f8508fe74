// bsdf_eval.hip — the batch BSDF entry: BSDFALL::sample / f / pdf
// (SceneTypes/BSDF.h:140-208) for an array of queries against a scene's
// materials, on the device (ctl_bsdf_eval, the uploaded scene) and on the host
// (ctl_host_bsdf_eval, a scene description).  Both run eval_query below, which
// calls the bsdf_sample / bsdf_f / bsdf_pdf dispatch of ctl_bsdf.h that
// shade_hit, the WavefrontPathTracer and the PrimTracer call, in its
// seven-type form.
#include <hip/hip_runtime.h>

#include <string>

#include "../../../include/ctl_trace.h"
#include "common.h"

using namespace ctl;

namespace {

// A query naming a material the scene does not have: zero value, sampled_type all ones.
CTL_HD ctl_bsdf_result eval_query(const ctl_material* mats, const ctl_material_ext* ext, uint32_t n_materials,
                                  const ctl_texture* textures, const uint32_t* tex_data, const ctl_bsdf_query& q) {
    ctl_bsdf_result r;
    r.value[0] = r.value[1] = r.value[2] = 0.0f;
    r.pdf = 0.0f;
    r.wo[0] = q.wo[0]; r.wo[1] = q.wo[1]; r.wo[2] = q.wo[2];
    r.sampled_type = 0xffffffffu;
    if (q.material >= n_materials) return r;
    const ctl_material* gm = mats + q.material;
    const ctl_material_ext* ge = ext ? ext + q.material : nullptr;   // read only by types 6-8, which upload / the host entry require it for
    const ctl_material mat = *gm;
    bsdf_rec b;
    b.wi = mk3(q.wi[0], q.wi[1], q.wi[2]);
    b.wo = mk3(q.wo[0], q.wo[1], q.wo[2]);
    b.sampled_type = 0;
    b.type_mask = q.type_mask;
    dgeom dg;
    dg.P = mk3s(0.0f);
    dg.sys.s = mk3(1.0f, 0.0f, 0.0f); dg.sys.t = mk3(0.0f, 1.0f, 0.0f); dg.sys.n = mk3(0.0f, 0.0f, 1.0f);
    dg.n = dg.sys.n;
    dg.dpdu = dg.sys.s; dg.dpdv = dg.sys.t;
    dg.uv = mk2(q.uv[0], q.uv[1]);
    dg.dudx = dg.dudy = dg.dvdx = dg.dvdy = 0.0f;
    dg.has_partials = false;
    const TexView tex{textures, tex_data};
    spec v = mk3s(0.0f);
    float pdf = 0.0f;
    if (q.op == CTL_BSDF_OP_SAMPLE) v = bsdf_sample<true>(mat, b, pdf, mk2(q.sample[0], q.sample[1]), dg, &tex, nullptr, gm, ge);
    else if (q.op == CTL_BSDF_OP_F) v = bsdf_f<true>(mat, b, dg, &tex, nullptr, gm, ge, (int)q.measure);
    else if (q.op == CTL_BSDF_OP_PDF) pdf = bsdf_pdf<true>(mat, b, gm, ge, (int)q.measure);
    r.value[0] = v.x; r.value[1] = v.y; r.value[2] = v.z;
    r.pdf = pdf;
    r.wo[0] = b.wo.x; r.wo[1] = b.wo.y; r.wo[2] = b.wo.z;
    r.sampled_type = b.sampled_type;
    return r;
}

__global__ __launch_bounds__(kBlock) void bsdf_eval_kernel(const ctl_material* mats, const ctl_material_ext* ext,
                                                           uint32_t n_materials, const ctl_texture* textures,
                                                           const uint32_t* tex_data, uint64_t n,
                                                           const ctl_bsdf_query* q, ctl_bsdf_result* out) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    out[i] = eval_query(mats, ext, n_materials, textures, tex_data, q[i]);
}

// The material checks of ctl_scene_upload that keep eval_query's reads in
// bounds, for a description that was never uploaded.
bool host_materials_ok(const ctl_scene_desc* d, std::string& err) {
    for (uint32_t i = 0; i < d->n_materials; i++) {
        const ctl_material& m = d->materials[i];
        const uint32_t t = m.bsdf_type;
        if (t != CTL_BSDF_DIFFUSE && (t < CTL_BSDF_DIELECTRIC || t > CTL_BSDF_PLASTIC)) {
            err = "host_bsdf_eval: material " + std::to_string(i) + ": unsupported BSDF type";
            return false;
        }
        if ((t == CTL_BSDF_CONDUCTOR || t == CTL_BSDF_ROUGHCONDUCTOR || t == CTL_BSDF_PLASTIC) && !d->materials_ext) {
            err = "host_bsdf_eval: material " + std::to_string(i) + " needs a ctl_material_ext record";
            return false;
        }
        if ((t == CTL_BSDF_ROUGHDIELECTRIC || t == CTL_BSDF_ROUGHCONDUCTOR) &&
            (m.distribution > CTL_MICROFACET_GGX || !m.sample_visible)) {
            err = "host_bsdf_eval: material " + std::to_string(i) + ": Beckmann/GGX with visible-normal sampling only";
            return false;
        }
        if (m.texture != 0xffffffffu && ((t != CTL_BSDF_DIFFUSE && t != CTL_BSDF_PLASTIC) || m.texture >= d->n_textures)) {
            err = "host_bsdf_eval: material " + std::to_string(i) + ": bad texture";
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

CTL_API ctl_status ctl_bsdf_eval(ctl_ctx* c, uint64_t n, const ctl_bsdf_query* d_queries, ctl_bsdf_result* d_results,
                                 void* stream) {
    if (!c) return CTL_ERR_INVALID;
    if (!c->has_scene) { c->err = "bsdf_eval: no scene uploaded"; return CTL_ERR_STATE; }
    if (n == 0) return CTL_OK;
    if (!d_queries || !d_results) { c->err = "bsdf_eval: null query or result array"; return CTL_ERR_INVALID; }
    const uint64_t blocks = (n + kBlock - 1) / kBlock;
    if (blocks > 0x7fffffffull) { c->err = "bsdf_eval: too many queries for one launch"; return CTL_ERR_INVALID; }
    if (hipSetDevice(c->device) != hipSuccess) { c->err = "bsdf_eval: hipSetDevice failed"; return CTL_ERR_HIP; }
    const DevScene& S = c->scene;
    const uint32_t n_materials = (uint32_t)(c->sarr[SA_MATS].bytes / sizeof(ctl_material));
    hipLaunchKernelGGL(bsdf_eval_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream),
                       S.mats, S.mats_ext, n_materials, S.textures, S.tex_data, n, d_queries, d_results);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { c->err = std::string("bsdf_eval: ") + hipGetErrorString(e); return CTL_ERR_HIP; }
    return CTL_OK;
}

CTL_API ctl_status ctl_host_bsdf_eval(const ctl_scene_desc* d, uint64_t n, const ctl_bsdf_query* queries,
                                      ctl_bsdf_result* results) {
    if (!d || (n && (!queries || !results))) { set_host_error("host_bsdf_eval: null argument"); return CTL_ERR_INVALID; }
    std::string err;
    if (!host_materials_ok(d, err)) { set_host_error(err); return CTL_ERR_INVALID; }
    for (uint64_t i = 0; i < n; i++)
        results[i] = eval_query(d->materials, d->materials_ext, d->n_materials, d->textures, d->tex_data, queries[i]);
    return CTL_OK;
}

}  // extern "C"
