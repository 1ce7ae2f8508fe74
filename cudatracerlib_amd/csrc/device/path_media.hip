// path_media.hip -- the PathTracer's kernels of the shading level kShadeMedia, in a code object of
// their own: the kernel templates of path_kernels.h instantiated for that level alone, behind the
// launches ctl_trace.hip hands over when its own levels do not hold the uploaded scene's.
#include "path_kernels.h"

namespace ctl {

bool media_launch_path(ctl_ctx* c, bool persistent, bool stats, const PathParams& P, const float* s1, const float2* s2,
                       uint64_t threads, uint64_t want, dim3 grid, unsigned long long* cursor, ctl_pixel* fb, SampleSlots PS,
                       uint32_t tbl, hipStream_t s) {
    return launch_path<kShadeMedia>(c, persistent, stats, P, s1, s2, threads, want, grid, cursor, fb, PS, tbl, s);
}

bool media_launch_blocks(ctl_ctx* c, const PathParams& P, const float* s1, const float2* s2, uint64_t items, uint64_t want,
                         unsigned long long* cursor, SampleSlots PS, const uint32_t* own_tbl, hipStream_t s) {
    return launch_path_blocks<kShadeMedia>(c, P, s1, s2, items, want, cursor, PS, own_tbl, s);
}

}  // namespace ctl
