// path_kernels.h -- the PathTracer's kernel templates (path_kernel, path_kernel_persistent,
// path_kernel_persistent_blocks, with the path state they park in LDS) and their one launch.
// Two files include it, each instantiating the levels of its own code object: ctl_trace.hip the
// levels lean ... lights, path_media.hip kShadeMedia alone, path_sensors.hip kShadeSensors alone.  There are
// several objects because the
// inliner's and the interprocedural passes' choices depend on a module's callers: with the media
// kernels in ctl_trace.hip's object, ten kernels of the levels full, env and alpha changed their
// spills; kShadeSensors follows that rule.  The kernels are in an anonymous namespace at file scope, so each object
// has its own.  ctl_trace.hip includes this in front of its own kernels (the sampler kernels come
// behind it): that order compiles every kernel to the code it had when all were in one file.
#pragma once
#include "common.h"

using namespace ctl;

#ifndef CTL_PERSIST_WAVES_FULL
#define CTL_PERSIST_WAVES_FULL 4   // ... with the C5 shading (out-of-line texture / microfacet / fp64 math
                                   // calls; path state parked in LDS): C5 3 waves 1480, 4 waves 1658 Mrays/s
#endif
#ifndef CTL_PERSIST_WAVES
#define CTL_PERSIST_WAVES 4   // waves/SIMD for the persistent path kernel, measured on C3 with the packed
                              // wide-node step: 2: 1576, 3: 1590, 4: 1666, 5: 1601, 6: 1505 Mrays/s
#endif

namespace {

// Path state of path_kernel_persistent parked in LDS while the lane's ray is
// traced: everything the shading needs and the traversal does not (throughput,
// radiance, last normal, wo, pixel position, BSDF pdf, depth and specular flag,
// the pending shadow ray's contribution, the sampler's sequence offsets and
// draw counters) -- 23 words per lane in [word][thread] layout (conflict-free
// ds_read/ds_write_b32).  Only the ray (origin, both directions, shadow
// distance) and a few flags stay in VGPRs across the traversal loop, so the
// traversal's register peak no longer stacks on top of the shading state.
// 16 KB stacks + 1 KB work words + 23 KB parked state = 40 KB per 256-thread
// block: 4 blocks per CU, i.e. the 4 waves/SIMD the VGPR budget targets.
// Lean kernel VGPR spills 36 -> 11; C3 2983 -> 3219 Mrays/s (profiles/r03_park_slack_ab.txt).
constexpr int kParkWords = 23;
// a block-list pass packs (work item, landing code 0..4) into the parked work item word
constexpr uint32_t kListItemBits = 29, kListItemMask = (1u << kListItemBits) - 1;
struct Park {
    int tid;
    __device__ __forceinline__ void put(int w, float x) const {
        ctl_lds_stack[kExtraLdsOff + w * kStackBlock + tid] = __float_as_int(x);
    }
    __device__ __forceinline__ void puti(int w, uint32_t x) const {
        ctl_lds_stack[kExtraLdsOff + w * kStackBlock + tid] = (int)x;
    }
    __device__ __forceinline__ float get(int w) const {
        return __int_as_float(ctl_lds_stack[kExtraLdsOff + w * kStackBlock + tid]);
    }
    __device__ __forceinline__ uint32_t geti(int w) const {
        return (uint32_t)ctl_lds_stack[kExtraLdsOff + w * kStackBlock + tid];
    }
    __device__ __forceinline__ void put3(int w, f3 x) const { put(w, x.x); put(w + 1, x.y); put(w + 2, x.z); }
    __device__ __forceinline__ f3 get3(int w) const { return mk3(get(w), get(w + 1), get(w + 2)); }
    __device__ __forceinline__ void store(const PathVars& v, const ShadowReq& sh, const SamplerDev& rng) const {
        put3(0, v.cl); put3(3, v.cf); put3(6, v.last_nor); put3(9, v.wo);
        put(12, v.pX.x); put(13, v.pX.y); put(14, v.brdf_pdf);
        puti(15, ((uint32_t)v.depth << 1) | (v.specular ? 1u : 0u));
        put3(16, sh.add);
        puti(19, rng.a); puti(20, rng.b); puti(21, rng.d1); puti(22, rng.d2);
    }
    // a new path (refill): everything but the shadow contribution, which only the
    // shadow phase reads and store_shaded always writes first -- so the previous
    // path's value is not carried through the loop just to be written here
    __device__ __forceinline__ void begin(const PathVars& v, const SamplerDev& rng) const {
        put3(0, v.cl); put3(3, v.cf); put3(6, v.last_nor); put3(9, v.wo);
        put(12, v.pX.x); put(13, v.pX.y); put(14, v.brdf_pdf);
        puti(15, ((uint32_t)v.depth << 1) | (v.specular ? 1u : 0u));
        puti(19, rng.a); puti(20, rng.b); puti(21, rng.d1); puti(22, rng.d2);
    }
    __device__ __forceinline__ void load(PathVars& v, ShadowReq& sh, SamplerDev& rng) const {
        v.cl = get3(0); v.cf = get3(3); v.last_nor = get3(6); v.wo = get3(9);
        v.pX.x = get(12); v.pX.y = get(13); v.brdf_pdf = get(14);
        const uint32_t ds = geti(15);
        v.depth = (int)(ds >> 1); v.specular = (ds & 1u) != 0;
        sh.add = get3(16);
        rng.a = geti(19); rng.b = geti(20); rng.d1 = geti(21); rng.d2 = geti(22);
    }
    // Partial loads and stores (the FULL kernels): after a trace the lane loads only
    // depth / specular and the sampler state; shade_hit reads the rest where it
    // is used (shading.h shade_hit, `pk`), and only what changed goes back.
    __device__ __forceinline__ void load_core(PathVars& v, SamplerDev& rng) const {
        const uint32_t ds = geti(15);
        v.depth = (int)(ds >> 1); v.specular = (ds & 1u) != 0;
        rng.a = geti(19); rng.b = geti(20); rng.d1 = geti(21); rng.d2 = geti(22);
    }
    __device__ __forceinline__ void load_px(PathVars& v) const { v.pX.x = get(12); v.pX.y = get(13); }
    __device__ __forceinline__ void load_mis(PathVars& v) const { v.brdf_pdf = get(14); v.last_nor = get3(6); }
    __device__ __forceinline__ void load_sample_state(PathVars& v) const { v.wo = get3(9); v.brdf_pdf = get(14); }
    __device__ __forceinline__ void load_cl_cf(PathVars& v) const { v.cl = get3(0); v.cf = get3(3); }
    __device__ __forceinline__ void store_cl(const PathVars& v) const { put3(0, v.cl); }
    __device__ __forceinline__ void store_depth(const PathVars& v) const {
        puti(15, ((uint32_t)v.depth << 1) | (v.specular ? 1u : 0u));
    }
    // after shade_hit: everything it can change (not the pixel position)
    __device__ __forceinline__ void store_shaded(const PathVars& v, const ShadowReq& sh, const SamplerDev& rng) const {
        put3(0, v.cl); put3(3, v.cf); put3(6, v.last_nor); put3(9, v.wo);
        put(14, v.brdf_pdf);
        store_depth(v);
        put3(16, sh.add);
        puti(21, rng.d1); puti(22, rng.d2);
    }
};

// dynamic LDS of path_kernel_persistent: lane stacks + the work item word per
// lane + the parked path state
constexpr size_t persistent_lds_bytes() {
    return kStackLdsBytes + sizeof(int) * kStackBlock * (1 + kParkWords);
}

// Megakernel schedule: PathTrace<true> (PathTracer.cu:10-113) with the
// traversals inline in the bounce, as the reference's pathKernel2 runs it.
template <bool STATS, bool SINGLE, int WIDE, int FULL>
struct PathCtx {
    const DevScene& S;
    const PathParams& P;
    SamplerDev& rng;
    LaneStack& st;
    uint32_t rays;
    TraceStats ts;
    bool ok;
    PathVars v;

    // one iteration of `while (depth++ < MaxPathLength)`; false = path done
    __device__ __forceinline__ bool bounce() {
        if (!(v.depth++ < P.max_path_length)) {
            // kShadeMedia: the loop ends with r2 still the miss a medium interaction went on from
            if constexpr (CTL_MEDIA_OF(FULL)) { if (v.vol_miss) v.cl = v.cl + env_miss<FULL>(S, P, v); }
            return false;
        }
        HitRec r2 = no_hit(FLT_MAX);   // traceRay (TraceHelper.cu:174-180)
        rays++;
        ok &= trace_one<0, STATS, SINGLE, WIDE, CTL_ALPHA_OF(FULL)>(S, v.rori, v.rdir, 0.0f, S.ray_eps, r2, st, &ts);
        ShadowReq sh;
        int ev = kMediumNone;
        if constexpr (CTL_MEDIA_OF(FULL)) {
            ev = medium_step<FULL>(S, P, rng, v, r2, sh);   // PathTracer.cu:24-58
            if (ev != kMediumNone) v.vol_miss = r2.tri == 0xffffffffu;
        }
        bool cont = ev == kMediumScattered;
        if (ev == kMediumNone) {
            if (r2.tri == 0xffffffffu) {
                v.cl = v.cl + env_miss<FULL>(S, P, v);   // PathTracer.cu:98-111
                return false;
            }
            if constexpr (CTL_MEDIA_OF(FULL)) v.vol_miss = false;
            cont = shade_hit<FULL, SINGLE>(S, P, rng, v, r2, sh);
        }
        if (sh.valid) {
            const bool any = P.shadow_any_hit != 0;
            HitRec h = no_hit(any ? sh.dist - S.ray_eps : FLT_MAX);
            rays++;
            if (any) ok &= trace_one<1, STATS, SINGLE, WIDE, CTL_ALPHA_OF(FULL)>(S, v.rori, sh.d, 0.0f, S.ray_eps, h, st, &ts,
                                                                                sh.dist);
            else ok &= trace_one<0, STATS, SINGLE, WIDE, CTL_ALPHA_OF(FULL)>(S, v.rori, sh.d, 0.0f, S.ray_eps, h, st, &ts);
            if (!shadow_occluded(S, any, h, sh.dist)) v.cl = v.cl + sh.add;
        }
        if constexpr (CTL_MEDIA_OF(FULL)) { if (ev == kMediumEnded && v.vol_miss) v.cl = v.cl + env_miss<FULL>(S, P, v); }
        return cont;
    }
};

// One path per thread (the reference's pathKernel2 launch shape).
template <bool STATS, bool SINGLE, int WIDE, int FULL>
__global__ __launch_bounds__(kBlock) void path_kernel(DevScene S_arg, PathParams P_arg, const float* s1, const float2* s2,
                                                      ctl_pixel* fb, unsigned long long* counters, SampleSlots PS) {
    const DevScene& S = kernarg_ref<DevScene>(S_arg, 0);   // read in place (common.h kernarg_ref)
    const PathParams& P = kernarg_ref<PathParams>(P_arg, kernarg_next<DevScene, PathParams>(0));
    CTL_LANE_STACK(st);
    const uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    uint32_t rays = 0;
    TraceStats ts{0, 0, 0};
    bool ok = true;
    uint32_t px, py;
    if (work_pixel(P, g, px, py)) {
        const uint32_t idx = py * P.width + px;   // TracerBase::getPixelIndex (Tracer.h:89-97)
        SamplerDev rng;
        rng.init(s1, s2, P.nseq, P.len, idx);
        PathCtx<STATS, SINGLE, WIDE, FULL> C{S, P, rng, st, 0, TraceStats{0, 0, 0}, true, PathVars{}};
        f3 o, dw;
        const f2 pX = primary_ray<FULL>(S, rng, px, py, o, dw);
        if (apron_keep(P, g, pX)) {
            C.v.begin(pX, o, dw);
            while (C.bounce()) {}
            store_sample(P, PS, 0, (uint32_t)g, px, py, pX, mk3s(1.0f) * C.v.cl);
        } else {
            PS.s[g] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // apron path landing outside the tile
        }
        rays = C.rays;
        ts = C.ts;
        ok = C.ok;
    } else if (g < PS.per_pass) {
        PS.s[g] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // work item outside the image: no sample
    }
    wave_add_u64(&counters[0], rays);
    // flush_counters written out: as a call, the STATS instantiations' registers change
    if (!ok) atomicAdd(&counters[1], 1ull);
    if (STATS) {
        wave_add_u64(&counters[2], ts.nodes);
        wave_add_u64(&counters[3], ts.tris);
        wave_add_u64(&counters[4], ts.inst);
    }
}

// Persistent path kernel with path regeneration (default schedule).  A
// resident grid of lanes, each owning one path at a time:
//  * every iteration a lane traces its pending ray to completion (extension
//    ray, or the NEE shadow ray of its last bounce) with one traversal call
//    site in the kernel, then shades / resolves it; the shadow ray is traced
//    right after the bounce that made it, so radiance sums happen in the
//    reference's order;
//  * a lane whose path ended stores its sample and takes the next work item
//    from a wave-aggregated 64-bit atomic cursor, so waves stay full through
//    the Russian-roulette tail instead of idling until their longest path
//    ends;
//  * the traverser is local to an iteration: only the path variables and the
//    pending ray are loop-carried, keeping the register peak low;
//  * tail hand-over (one-instance kernels, CTL_TAIL_LANES): once a ray of the
//    iteration has finished and only a few lanes still traverse, the wave leaves
//    the trace; those lanes write their traversal state above their stack top
//    and go on in the next iteration, beside the rays the others start meanwhile.
//    A ray's visit order does not depend on where its rounds are cut.
// Work items are independent (own sampler index, own sample slot), so the
// framebuffer is bit-identical to path_kernel's.
// The loop is persistent_loop.h, the body of two kernel templates so that the
// default kernels keep their names and code: path_kernel_persistent (ownership
// tile % num_ranks == rank) and path_kernel_persistent_blocks (the blocks of a
// list, ctl_render_pass_blocks).
// One work item of ctl_camera_rays, the body of camera_ray_kernel (ctl_trace.hip) and of camera_ray_sensors_kernel
// (path_sensors.hip): the path kernels' first ray (primary_ray of the level) as a traversalRay, tmin = scene eps,
// tmax = FLT_MAX; a work item outside the image gets an empty interval (tmax = 0).  items <= the caller's capacity.
template <int FULL>
__device__ __forceinline__ void camera_ray_item(const DevScene& S, const PathParams& P, const float* s1, const float2* s2,
                                                uint64_t items, ctl_ray* rays) {
    const uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= items) return;
    uint32_t px, py;
    float4 o4 = make_float4(0.0f, 0.0f, 0.0f, S.ray_eps), d4 = make_float4(0.0f, 0.0f, 1.0f, 0.0f);
    if (work_pixel(P, g, px, py)) {
        const uint32_t idx = py * P.width + px;
        SamplerDev rng;
        rng.init(s1, s2, P.nseq, P.len, idx);
        f3 o, d;
        (void)primary_ray<FULL>(S, rng, px, py, o, d);
        o4 = make_float4(o.x, o.y, o.z, S.ray_eps);
        d4 = make_float4(d.x, d.y, d.z, FLT_MAX);
    }
    float4* r4 = reinterpret_cast<float4*>(rays + g);
    r4[0] = o4;
    r4[1] = d4;
}

#define CTL_PERSIST_KERNEL_ATTRS \
    __global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(SINGLE ? (FULL ? CTL_PERSIST_WAVES_FULL : CTL_PERSIST_WAVES) : 2)))

template <bool STATS, bool SINGLE, int WIDE, int FULL>
CTL_PERSIST_KERNEL_ATTRS void path_kernel_persistent(DevScene S_arg, PathParams P_arg, const float* s1, const float2* s2,
                                                     uint64_t items, unsigned long long* cursor,
                                                     unsigned long long* counters, SampleSlots PS, uint32_t tbl) {
    using OWN = OwnModulo;
    const uint32_t* const own_tbl = nullptr;
#include "persistent_loop.h"
}

// A block-list pass: one pass per launch (tbl = 0), no traversal statistics.
template <bool SINGLE, int WIDE, int FULL>
CTL_PERSIST_KERNEL_ATTRS void path_kernel_persistent_blocks(DevScene S_arg, PathParams P_arg, const float* s1,
                                                            const float2* s2, uint64_t items, unsigned long long* cursor,
                                                            unsigned long long* counters, SampleSlots PS,
                                                            const uint32_t* __restrict__ own_tbl) {
    using OWN = OwnList;
    constexpr bool STATS = false;
    constexpr uint32_t tbl = 0;
#include "persistent_loop.h"
}
#undef CTL_PERSIST_KERNEL_ATTRS

#ifndef CTL_PERSIST_BPC
#define CTL_PERSIST_BPC 0   // resident blocks per CU of the persistent path kernel (0: occupancy limit)
#endif

// Host: the launch of one pass's path kernel, and of a block-list pass's, for the uploaded scene's
// tree and shading level.  L... are the levels the including file instantiates; false, and nothing
// launched, when the scene's level is not among them.
template <int... L>
bool launch_path(ctl_ctx* c, bool persistent, bool stats, const PathParams& P, const float* s1, const float2* s2,
                 uint64_t threads, uint64_t want, dim3 grid, unsigned long long* cursor, ctl_pixel* fb, SampleSlots PS,
                 uint32_t tbl, hipStream_t s) {
    bool known = false;
    with_tree(stats, c->scene.single != 0, c->scene.wide != 0, [&](auto ST, auto SG, auto WD) {
        known = with_level<L...>((int)c->scene.full_shading, [&](auto FU) {
            if (persistent) {
                constexpr size_t lds = persistent_lds_bytes();
                auto k = path_kernel_persistent<decltype(ST)::value, decltype(SG)::value, decltype(WD)::value,
                                                decltype(FU)::value>;
                hipLaunchKernelGGL(k, resident_grid(c, k, lds, want, CTL_PERSIST_BPC), dim3(kBlock), lds, s, c->scene,
                                   P, s1, s2, threads, cursor, c->d_counters, PS, tbl);
            } else {
                auto k = path_kernel<decltype(ST)::value, decltype(SG)::value, decltype(WD)::value,
                                     decltype(FU)::value>;
                hipLaunchKernelGGL(k, grid, dim3(kBlock), kStackLdsBytes, s, c->scene, P, s1, s2, fb, c->d_counters,
                                   PS);
            }
        });
    });
    return known;
}

template <int... L>
bool launch_path_blocks(ctl_ctx* c, const PathParams& P, const float* s1, const float2* s2, uint64_t items,
                        uint64_t want, unsigned long long* cursor, SampleSlots PS, const uint32_t* own_tbl,
                        hipStream_t s) {
    bool known = false;
    with_tree(c->scene.single != 0, c->scene.wide != 0, [&](auto SG, auto WD) {
        known = with_level<L...>((int)c->scene.full_shading, [&](auto FU) {
            constexpr size_t lds = persistent_lds_bytes();
            auto k = path_kernel_persistent_blocks<decltype(SG)::value, decltype(WD)::value, decltype(FU)::value>;
            hipLaunchKernelGGL(k, resident_grid(c, k, lds, want, CTL_PERSIST_BPC), dim3(kBlock), lds, s, c->scene, P,
                               s1, s2, items, cursor, c->d_counters, PS, own_tbl);
        });
    });
    return known;
}

}  // namespace
