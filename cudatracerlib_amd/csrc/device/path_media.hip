// path_media.hip -- the PathTracer's kernels of the shading level kShadeMedia (shading.h), in a code
// object of their own: the kernel templates of ctl_trace.hip compiled for that level alone, and the
// launches ctl_trace.hip hands over when the uploaded scene has a volume.
#define CTL_PATH_KERNELS_ONLY
#include "ctl_trace.hip"

#ifndef CTL_PERSIST_BPC
#define CTL_PERSIST_BPC 0   // as in ctl_trace.hip
#endif

namespace ctl {

void media_launch_path(ctl_ctx* c, bool persistent, bool stats, const PathParams& P, const float* s1, const float2* s2,
                       uint64_t threads, uint64_t want, dim3 grid, unsigned long long* cursor, ctl_pixel* fb, SampleSlots PS,
                       uint32_t tbl, hipStream_t s) {
    with_tree(stats, c->scene.single != 0, c->scene.wide != 0, [&](auto ST, auto SG, auto WD) {
        if (persistent) {
            constexpr size_t lds = persistent_lds_bytes();
            auto k = path_kernel_persistent<decltype(ST)::value, decltype(SG)::value, decltype(WD)::value, kShadeMedia>;
            hipLaunchKernelGGL(k, resident_grid(c, k, lds, want, CTL_PERSIST_BPC), dim3(kBlock), lds, s, c->scene, P, s1,
                               s2, threads, cursor, c->d_counters, PS, tbl);
        } else {
            auto k = path_kernel<decltype(ST)::value, decltype(SG)::value, decltype(WD)::value, kShadeMedia>;
            hipLaunchKernelGGL(k, grid, dim3(kBlock), kStackLdsBytes, s, c->scene, P, s1, s2, fb, c->d_counters, PS);
        }
    });
}

void media_launch_blocks(ctl_ctx* c, const PathParams& P, const float* s1, const float2* s2, uint64_t items, uint64_t want,
                         unsigned long long* cursor, SampleSlots PS, const uint32_t* own_tbl, hipStream_t s) {
    with_tree(c->scene.single != 0, c->scene.wide != 0, [&](auto SG, auto WD) {
        constexpr size_t lds = persistent_lds_bytes();
        auto k = path_kernel_persistent_blocks<decltype(SG)::value, decltype(WD)::value, kShadeMedia>;
        hipLaunchKernelGGL(k, resident_grid(c, k, lds, want, CTL_PERSIST_BPC), dim3(kBlock), lds, s, c->scene, P, s1, s2,
                           items, cursor, c->d_counters, PS, own_tbl);
    });
}

}  // namespace ctl
