// path_sensors.hip -- the PathTracer's kernels of the shading level kShadeSensors, in a code object of
// their own as path_media.hip's are: the kernel templates of path_kernels.h instantiated for that level
// alone, behind the launches ctl_trace.hip hands over when neither its own levels nor path_media.hip's
// hold the uploaded scene's; and that level's camera-ray batch (ctl_camera_rays), kept out of
// ctl_trace.hip's object for the same reason.
#include "path_kernels.h"

namespace {

// camera_ray_kernel (ctl_trace.hip) with the scene's sensor
__global__ __launch_bounds__(kBlock) void camera_ray_sensors_kernel(DevScene S_arg, PathParams P_arg, const float* s1,
                                                                    const float2* s2, uint64_t items, ctl_ray* rays) {
    const DevScene& S = kernarg_ref<DevScene>(S_arg, 0);   // read in place (common.h kernarg_ref)
    const PathParams& P = kernarg_ref<PathParams>(P_arg, kernarg_next<DevScene, PathParams>(0));
    camera_ray_item<kShadeSensors>(S, P, s1, s2, items, rays);
}

}  // namespace

namespace ctl {

bool sensors_launch_path(ctl_ctx* c, bool persistent, bool stats, const PathParams& P, const float* s1, const float2* s2,
                         uint64_t threads, uint64_t want, dim3 grid, unsigned long long* cursor, ctl_pixel* fb,
                         SampleSlots PS, uint32_t tbl, hipStream_t s) {
    return launch_path<kShadeSensors>(c, persistent, stats, P, s1, s2, threads, want, grid, cursor, fb, PS, tbl, s);
}

bool sensors_launch_blocks(ctl_ctx* c, const PathParams& P, const float* s1, const float2* s2, uint64_t items,
                           uint64_t want, unsigned long long* cursor, SampleSlots PS, const uint32_t* own_tbl,
                           hipStream_t s) {
    return launch_path_blocks<kShadeSensors>(c, P, s1, s2, items, want, cursor, PS, own_tbl, s);
}

bool sensors_launch_camera_rays(ctl_ctx* c, const PathParams& P, const float* s1, const float2* s2, uint64_t items,
                                ctl_ray* rays, hipStream_t s) {
    if (!CTL_SENSORS_OF((int)c->scene.full_shading)) return false;
    hipLaunchKernelGGL(camera_ray_sensors_kernel, dim3((unsigned)((items + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                       c->scene, P, s1, s2, items, rays);
    return true;
}

}  // namespace ctl
