// sensor_eval.hip — the batch sensor entry: Sensor::sampleRay and
// Sensor::sampleRayDifferential (SceneTypes/Sensor.cu) for an array of queries
// against a scene's sensor, on the device (ctl_sensor_eval, the uploaded scene)
// and on the host (ctl_host_sensor_eval, a scene description).  Both run
// eval_query below, which calls the two inline functions of ctl_sensor.h that
// the integrators' camera stages call (shading.h primary_ray and
// sensor_partials, prim.hip, wpt.hip).
#include <hip/hip_runtime.h>

#include <string>

#include "../../../include/ctl_trace.h"
#include "common.h"

using namespace ctl;

namespace {

CTL_HD void put3(float out[3], f3 v) { out[0] = v.x; out[1] = v.y; out[2] = v.z; }

CTL_HD ctl_sensor_result eval_query(const ctl_camera& C, const ctl_sensor& R, const ctl_sensor_query& q) {
    ctl_sensor_result r;
    const f2 pX = mk2(q.pixel_sample[0], q.pixel_sample[1]), ap = mk2(q.aperture_sample[0], q.aperture_sample[1]);
    f3 o, d, oX = mk3s(0.0f), dX = mk3s(0.0f), oY = mk3s(0.0f), dY = mk3s(0.0f);
    bool has = false;
    if (q.differential) has = sensor_sample_ray_differential(C, R, pX, ap, o, d, oX, dX, oY, dY);
    else sensor_sample_ray(C, R, pX, ap, o, d);
    if (!has) oX = dX = oY = dY = mk3s(0.0f);
    put3(r.o, o); put3(r.d, d);
    put3(r.ox, oX); put3(r.dx, dX);
    put3(r.oy, oY); put3(r.dy, dY);
    r.has_differentials = has ? 1u : 0u;
    r.pad = 0;
    return r;
}

// the camera by value (a kernel argument), the record where the kernels read it (traverse.h scene_sensor)
__global__ __launch_bounds__(kBlock) void sensor_eval_kernel(ctl_camera C, const ctl_sensor* R, uint64_t n,
                                                             const ctl_sensor_query* q, ctl_sensor_result* out) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    out[i] = eval_query(C, *R, q[i]);
}

}  // namespace

namespace ctl {
void set_host_error(const std::string& s);   // host/scene.cpp
}

extern "C" {

CTL_API ctl_status ctl_sensor_eval(ctl_ctx* c, const ctl_sensor_query* d_queries, int64_t n, ctl_sensor_result* d_results,
                                   void* stream) {
    if (!c) return CTL_ERR_INVALID;
    if (!c->has_scene) { c->err = "sensor_eval: no scene uploaded"; return CTL_ERR_STATE; }
    if (n < 0) { c->err = "sensor_eval: negative query count"; return CTL_ERR_INVALID; }
    if (n == 0) return CTL_OK;
    if (!d_queries || !d_results) { c->err = "sensor_eval: null query or result array"; return CTL_ERR_INVALID; }
    const uint64_t blocks = ((uint64_t)n + kBlock - 1) / kBlock;
    if (blocks > 0x7fffffffull) { c->err = "sensor_eval: too many queries for one launch"; return CTL_ERR_INVALID; }
    if (hipSetDevice(c->device) != hipSuccess) { c->err = "sensor_eval: hipSetDevice failed"; return CTL_ERR_HIP; }
    const ctl_sensor* rec =
        reinterpret_cast<const ctl_sensor*>(reinterpret_cast<const char*>(c->scene.lights) + kSensorAt);
    hipLaunchKernelGGL(sensor_eval_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream),
                       c->scene.camera, rec, (uint64_t)n, d_queries, d_results);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { c->err = std::string("sensor_eval: ") + hipGetErrorString(e); return CTL_ERR_HIP; }
    return CTL_OK;
}

CTL_API ctl_status ctl_host_sensor_eval(const ctl_scene_desc* d, const ctl_sensor_query* queries, int64_t n,
                                        ctl_sensor_result* results) {
    if (!d || n < 0 || (n && (!queries || !results))) { set_host_error("host_sensor_eval: invalid argument"); return CTL_ERR_INVALID; }
    const ctl_sensor R = d->sensor ? *d->sensor : sensor_default();
    if (const char* why = sensor_check(R)) { set_host_error(std::string("host_sensor_eval: ") + why); return CTL_ERR_INVALID; }
    for (int64_t i = 0; i < n; i++) results[i] = eval_query(d->camera, R, queries[i]);
    return CTL_OK;
}

}  // extern "C"
