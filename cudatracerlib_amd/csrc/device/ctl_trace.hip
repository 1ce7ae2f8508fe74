// ctl_trace.hip — gfx950 kernels and the device half of the C ABI
// (include/ctl_trace.h).
//
//   intersect_kernel   batch closest/any hit over ctl_ray -> ctl_hit
//                      (intersectKernel<ANY_HIT> + __internal__IntersectBuffers,
//                       Kernel/TraceHelper.cu:326-746)
//   path_kernel_persistent  one PathTracer pass (default schedule): resident
//                      grid, path regeneration from an atomic pixel cursor
//   path_kernel        one PathTracer pass, one thread per pixel path
//                      (both: sensor ray + PathTrace<true> + AddSample;
//                       pathKernel2 / PathTrace, Integrators/PathTracer.cu:10-113,182-194;
//                       Image::AddSample, Engine/Image.cu:22-44)
//   fold_blocks_kernel the sample fold of a block-list pass (ctl_render_pass_blocks:
//                      path_kernel_persistent_blocks, the persistent loop with the
//                      OwnList ownership policy, common.h)
//   sampler_kernel     SequenceSamplerData tables of a pass (Sampler.cu, CudaRandom.cu)
// The path kernel templates (path_kernel, path_kernel_persistent, path_kernel_persistent_blocks) and
// their launch are path_kernels.h, instantiated here for every shading level but kShadeMedia and kShadeSensors
// (path_media.hip).  The wavefront schedule lives in wavefront.hip.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../../include/ctl_trace.h"
#include "../host/bvh_wide.h"
#include "../ctl_qnode.h"
#include "common.h"

namespace ctl {
void sampler_tables(uint64_t pass, uint32_t nseq, uint32_t len, float* seq1d, float* seq2d);
void sampler_pass_state(uint64_t pass, uint32_t nseq, uint32_t len, uint32_t v[5], uint32_t* d);
void sampler_step_powers(uint32_t* out, int kmax);
void sampler_seq_powers(uint32_t* out, uint32_t len);
}

using namespace ctl;

static_assert(sizeof(ctl_bvh_node) == 64, "BVHNodeData is 64 B");
static_assert(sizeof(ctl_woop_tri) == 48, "TriIntersectorData is 48 B");
static_assert(sizeof(ctl_triangle_data) == 32, "TriangleData is 32 B");
static_assert(sizeof(ctl_kernel_mesh) == 20, "KernelMesh is 20 B");
static_assert(sizeof(ctl_node) == 24, "Node is 24 B");
static_assert(sizeof(ctl_ray) == 32, "traversalRay is 32 B");
static_assert(sizeof(ctl_hit) == 16, "traversalResult is 16 B");
static_assert(sizeof(ctl_pixel) == 28, "PixelData is 28 B");
static_assert(sizeof(ctl_light_tri) == 64, "ShapeSet::triData is 64 B");
static_assert(sizeof(ctl_material) == 80, "ctl_material is 80 B");
static_assert(sizeof(ctl_texture) == 380, "ctl_texture is 380 B");
static_assert(sizeof(ctl_pixel_variance) == 44, "PixelVarianceInfo is 44 B");

#include "path_kernels.h"
// the levels whose path kernels this object holds; kShadeMedia's are path_media.hip's (ctl::media_launch_*),
// kShadeSensors' path_sensors.hip's (ctl::sensors_launch_*)
#define CTL_PATH_LEVELS_HERE kShadeLean, kShadeFull, kShadeEnv, kShadeAlpha, kShadeMat, kShadeLights

namespace {

// SequenceSamplerData tables of one pass generated on the device: sequence q
// starts q*len*3 draws after the pass's first state (host-computed), reached
// with the GF(2) step powers M^(2^k); then curand_uniform * (1 - 1e-5f)
// exactly as Base/CudaRandom.cu:8-17 and the CUDA toolkit's XORWOW.
constexpr int kJumpBits = 24;
struct XorwowDev { uint32_t v[5]; uint32_t d; };

// One wave per sequence: the GF(2) matrix-vector product of each jump is
// split over the lanes by input bit (lane j holds state bits j, j+64, j+128)
// and XOR-reduced across the wave, so a jump costs one round of column loads
// and a 6-step butterfly instead of ~80 dependent column loads on one lane.
__device__ __forceinline__ uint32_t wave_xor(uint32_t x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x ^= (uint32_t)__shfl_xor((int)x, m);
    return x;
}

// powers: [kJumpBits] M^(2^k), then (sampler_seq_powers) [64] A^ql and
// [64] A^(64 qh) with A = M^(3 len), then M^len and M^(len + 2 (len / 2)), all 800 words.
// Sequence q < 4096 jumps in two rounds (A^ql, A^(64 qh)); a larger q by the
// binary powers of its offset.  The rounds are dependent memory round trips,
// so two instead of the ~10 set bits of q * 3 len is what the kernel's time is
// made of (30.6 -> 18.4 us per pass).  Then three lanes draw a third of the
// sequence each, from the states len and len + 2 (len / 2) steps on (one more round each,
// independent of each other): lane 0 the 1-D values, lanes 1 and 2 the first
// and second half of the 2-D pairs.
constexpr int kSeqPowBase = kJumpBits * 800;
// v <- M v over the wave (lane j holds input bits j, j + 64, j + 128)
__device__ __forceinline__ void wave_apply(const uint32_t* __restrict__ M, uint32_t v[5], int lane) {
    const bool lo = lane < 32;
    const uint32_t sh = (uint32_t)(lane & 31);
    const uint32_t w0 = lo ? v[0] : v[1], w1 = lo ? v[2] : v[3];
    uint32_t r0 = 0, r1 = 0, r2 = 0, r3 = 0, r4 = 0;
    auto col = [&](uint32_t word, int b) {
        if ((word >> sh) & 1u) {
            const uint32_t* c = M + b * 5;
            r0 ^= c[0]; r1 ^= c[1]; r2 ^= c[2]; r3 ^= c[3]; r4 ^= c[4];
        }
    };
    col(w0, lane);
    col(w1, lane + 64);
    if (lo) col(v[4], lane + 128);
    v[0] = wave_xor(r0); v[1] = wave_xor(r1); v[2] = wave_xor(r2); v[3] = wave_xor(r3); v[4] = wave_xor(r4);
}

__device__ __forceinline__ void sampler_sequence(const uint32_t* __restrict__ powers, const XorwowDev& base,
                                                 uint32_t nseq, uint32_t len, float* s1, float2* s2) {
    const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (q >= nseq) return;   // whole wave
    const uint32_t off = q * len * 3;
    uint32_t v[5] = {base.v[0], base.v[1], base.v[2], base.v[3], base.v[4]};
    const bool twoStep = q < 4096u;
    for (int k = 0; k < (twoStep ? 2 : kJumpBits); k++) {
        const uint32_t* M;
        if (twoStep) {
            const uint32_t digit = k == 0 ? (q & 63u) : (q >> 6);
            if (!digit) continue;   // identity; uniform over the wave
            M = powers + kSeqPowBase + (k * 64 + digit) * 800;
        } else {
            if (!((off >> k) & 1u)) continue;   // uniform over the wave
            M = powers + k * 800;
        }
        wave_apply(M, v, lane);
    }
    // the states len and len + 2 (len / 2) draws on, for lanes 1 and 2
    uint32_t va[5] = {v[0], v[1], v[2], v[3], v[4]}, vb[5] = {v[0], v[1], v[2], v[3], v[4]};
    wave_apply(powers + kSeqPowBase + 128 * 800, va, lane);
    wave_apply(powers + kSeqPowBase + 129 * 800, vb, lane);
    if (lane > 2) return;
    uint32_t start = 0;
    if (lane == 1) { for (int w = 0; w < 5; w++) v[w] = va[w]; start = len; }
    if (lane == 2) { for (int w = 0; w < 5; w++) v[w] = vb[w]; start = len + 2 * (len / 2); }
    uint32_t d = base.d + 362437u * (off + start);
    auto next = [&]() -> float {
        uint32_t t = v[0] ^ (v[0] >> 2);
        v[0] = v[1]; v[1] = v[2]; v[2] = v[3]; v[3] = v[4];
        v[4] = (v[4] ^ (v[4] << 4)) ^ (t ^ (t << 1));
        d += 362437u;
        const float kInv = 2.3283064e-10f;
        float f = (float)(v[4] + d) * kInv + (kInv / 2.0f);
        return f * (1 - 1e-5f);
    };
    if (lane == 0) {
        for (uint32_t i = 0; i < len; i++) s1[i * nseq + q] = next();
    } else {
        // lane 1: pairs 0 .. len/2 - 1 (draws len .. len + 2 (len / 2) - 1); lane 2: the rest
        const uint32_t i0 = lane == 1 ? 0u : len / 2, i1 = lane == 1 ? len / 2 : len;
        for (uint32_t i = i0; i < i1; i++) {
            float x = next();
            float y = next();
            s2[i * nseq + q] = make_float2(x, y);
        }
    }
}

__global__ __launch_bounds__(256) void sampler_kernel(const uint32_t* __restrict__ powers, XorwowDev base,
                                                      uint32_t nseq, uint32_t len, float* s1, float2* s2) {
    sampler_sequence(powers, base, nseq, len, s1, s2);
}

// The tables of up to kSamplerBatch passes in one launch (ctl_render_passes):
// blockIdx.y = pass slot, whose first state is B.b[slot] and whose tables
// start slot * tbl elements in.  One launch keeps the GPU busier than a chain
// of single-pass launches of 4096 waves each (latency-bound jump rounds).
constexpr uint32_t kSamplerBatch = 128;
struct SamplerBases { XorwowDev b[kSamplerBatch]; };
static_assert(sizeof(SamplerBases) <= 3584, "sampler bases must fit the 4 KB kernel-argument segment");
__global__ __launch_bounds__(256) void sampler_batch_kernel(const uint32_t* __restrict__ powers, SamplerBases B,
                                                            uint32_t nseq, uint32_t len, float* s1, float2* s2,
                                                            uint64_t tbl) {
    const uint32_t slot = blockIdx.y;
    sampler_sequence(powers, B.b[slot], nseq, len, s1 + slot * tbl, s2 + slot * tbl);
}

// Batch closest/any hit (intersectKernel<ANY_HIT>, TraceHelper.cu:326-734):
// ray tmin bounds both the node spans and the triangle test (:650).  Resident
// grid; lanes whose ray finished take the next ray from a wave-aggregated
// atomic cursor between traversal rounds (the reference fetches per warp per
// batch of 32 rays, :379-399), so waves stay full on incoherent rays.
template <int ANY, bool STATS, bool SINGLE, int WIDE>
// Two segments (rays, hits)[0, n) then (rays2, hits2)[0, n2) in one launch: the
// wavefront tracer's payload and secondary batches share one resident grid and
// one tail.  ANY: 0 closest hit, 1 any hit (intersectKernel<true>, culled at the
// ray's tmax), 2 closest hit for the first segment and, for the second, the
// shadow query (any hit below tmax, boxes culled at tmax + slab_slack: the
// WavefrontPathTracer's CTL_WPT_SHADOW_ANY_HIT).
#ifndef CTL_REFILL_MIN
#define CTL_REFILL_MIN 40   // batch traversal: refill once at least this many lanes of the wave wait for a ray
                           // (C3 WPT sweep 1/8/24/32/40/48/56: 1093/1222/1505/1563/1564/1569/1545 Mrays/s)
#endif
__global__ __launch_bounds__(kBlock) void intersect_kernel(DevScene S_arg, int64_t n, const ctl_ray* rays, ctl_hit* hits,
                                                           int64_t n2, const ctl_ray* rays2, ctl_hit* hits2,
                                                           unsigned long long* cursor, unsigned long long* counters,
                                                           const uint32_t* dcount, uint32_t band_w) {
    const DevScene& S = kernarg_ref<DevScene>(S_arg, 0);   // read in place (common.h kernarg_ref)
    // dcount: the two segment sizes read from device memory (the WavefrontPathTracer's
    // queue counts, written by the previous bounce's scan: no host round trip); the
    // batch is then counted here as traced rays
    if (dcount) {
        n = dcount[0];
        n2 = dcount[1];
        if (blockIdx.x == 0 && threadIdx.x == 0 && n + n2 > 0) atomicAdd(&counters[0], (unsigned long long)(n + n2));
    }
    const int64_t total = n + n2;
    CTL_LANE_STACK(st);
    TraceStats ts{0, 0, 0};
    Traverser<ANY, STATS, SINGLE, WIDE> T;
    T.done = true;
    bool haveRay = false, exhausted = false, ovf = false, seg2 = false;
    int64_t ray = 0;   // slot in its segment
    while (true) {
        if (haveRay && T.done) {
            uint4 res = make_uint4((uint32_t)__float_as_int(T.h.t), 0xffffffffu, 0xffffffffu, 0u);
            if (T.h.tri != 0xffffffffu) {   // TraceHelper.cu:722-731
                res.y = T.h.node;
                res.z = T.h.tri;
                uint16_t xd = (uint16_t)(T.h.u * 65535), yd = (uint16_t)(T.h.v * 65535);
                res.w = ((uint32_t)yd << 16) | (uint32_t)xd;
            }
            reinterpret_cast<uint4*>(seg2 ? hits2 + ray : hits + ray)[0] = res;
            ovf |= st.overflow;
            haveRay = false;
        }
        const bool need = !haveRay && !exhausted;
        const uint64_t mask = __ballot(need);
        if (mask && (__popcll(mask) >= CTL_REFILL_MIN || !__any(haveRay))) {
            const unsigned long long slot = wave_claim(cursor, mask);
            if (need) {
                int64_t k = (int64_t)slot;
                if (k < total) {
                    // band_w: the first segment is a row-major image of that width (the
                    // WavefrontPathTracer's camera rays); trace it in 8-row bands, column by
                    // column, so a wave's 64 rays form an 8 x 8 block (hits go to their own
                    // slots, so the results are those of row order)
                    if (band_w && k < n) {
                        const int64_t bw = 8 * (int64_t)band_w, band = k / bw, h = n / band_w;
                        const int64_t bh = h - 8 * band < 8 ? h - 8 * band : 8, r = k - band * bw;
                        k = (8 * band + r % bh) * band_w + r / bh;
                    }
                    seg2 = k >= n;
                    ray = seg2 ? k - n : k;
                    haveRay = true;
                    const float4* r4 = reinterpret_cast<const float4*>(seg2 ? rays2 + ray : rays + ray);
                    const float4 o = r4[0], d = r4[1];
                    if (ANY == 2) T.anyhit = seg2;
                    T.init(S, mk3(o.x, o.y, o.z), mk3(d.x, d.y, d.z), o.w, o.w, d.w, st, &ts,
                           ANY == 2 && seg2 ? d.w : -1.0f);
                } else {
                    exhausted = true;
                }
            }
        }
        if (!__any(haveRay)) break;
        if (haveRay && !T.done) T.round(S, st, &ts);
    }
    flush_counters<STATS>(counters, ovf, ts);
}

// Primary rays of one pass in work order (the path kernels' first ray: pixel
// jitter + aperture draw + PerspectiveSensor, Sensor.cu:130-144), as a
// traversalRay batch: tmin = scene eps, tmax = FLT_MAX.  Work items outside
// the image get an empty interval (tmax = 0).
__global__ __launch_bounds__(kBlock) void camera_ray_kernel(DevScene S_arg, PathParams P_arg, const float* s1, const float2* s2,
                                                            uint64_t items, ctl_ray* rays) {
    const DevScene& S = kernarg_ref<DevScene>(S_arg, 0);   // read in place (common.h kernarg_ref)
    const PathParams& P = kernarg_ref<PathParams>(P_arg, kernarg_next<DevScene, PathParams>(0));
    camera_ray_item<kShadeLean>(S, P, s1, s2, items, rays);   // path_kernels.h
}

// Batch KernelDynamicScene::Occluded(Ray(o, d), 0, tmax) (KernelDynamicScene.cu:70-80),
// tmax = the ray's d.w (o.w ignored), with the path kernels' semantics: the
// reference's closest-hit form (ANYQ false) or the any-hit query of
// shadow_any_hit = 1 (boxes culled at tmax + slab_slack, traverse.h).  traceRay flavour: span tmin
// 0, triangles t > eps, the alpha test when the scene has alpha maps.  One ray
// per lane: a checker and a drop-in for callers of Occluded, not a hot path.
template <bool ANYQ, bool SINGLE, int WIDE>
__global__ __launch_bounds__(kBlock) void occluded_kernel(DevScene S_arg, int64_t n, const ctl_ray* rays, uint32_t* out,
                                                          unsigned long long* counters) {
    const DevScene& S = kernarg_ref<DevScene>(S_arg, 0);   // read in place (common.h kernarg_ref)
    CTL_LANE_STACK(st);
    TraceStats ts{0, 0, 0};
    const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= n) return;
    const float4* r4 = reinterpret_cast<const float4*>(rays + g);
    const float4 o = r4[0], d = r4[1];
    const float dist = d.w;
    HitRec h = no_hit(ANYQ ? dist - S.ray_eps : FLT_MAX);
    bool ok = true;
    if (S.n_nodes != 0)
        ok = trace_one<ANYQ ? 1 : 0, false, SINGLE, WIDE, true>(S, mk3(o.x, o.y, o.z), mk3(d.x, d.y, d.z), 0.0f,
                                                               S.ray_eps, h, st, &ts, ANYQ ? dist : -1.0f);
    out[g] = shadow_occluded(S, ANYQ, h, dist) ? 1u : 0u;
    if (!ok) atomicAdd(&counters[1], 1ull);
}

}  // namespace

// ===========================================================================
// Context + C ABI
// ===========================================================================
static std::mutex g_err_mtx;
static std::string g_create_err;

extern "C" {

CTL_API int32_t ctl_abi_version(void) { return CTL_ABI_VERSION; }

CTL_API const char* ctl_last_error(const ctl_ctx* ctx) {
    if (ctx) return ctx->err.c_str();
    std::lock_guard<std::mutex> g(g_err_mtx);
    return g_create_err.c_str();
}

CTL_API ctl_ctx* ctl_create(int32_t device) {
    ctl_ctx* c = nullptr;
    auto fail = [&c](const std::string& s) -> ctl_ctx* {
        ctl_destroy(c);   // frees what the context already owns
        std::lock_guard<std::mutex> g(g_err_mtx);
        g_create_err = s;
        return nullptr;
    };
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail("ctl_create: no HIP device");
    if (device < 0 || device >= n) return fail("ctl_create: device index out of range");
    if (hipSetDevice(device) != hipSuccess) return fail("ctl_create: hipSetDevice failed");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return fail("ctl_create: hipGetDeviceProperties failed");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(std::string("ctl_create: device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
    c = new ctl_ctx();
    c->device = device;
    c->cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (c->fixed.alloc(&c->d_counters, 16) != hipSuccess ||
        hipMemset(c->d_counters, 0, 16 * sizeof(unsigned long long)) != hipSuccess)
        return fail("ctl_create: counter allocation failed");
    if (c->fixed.alloc(&c->d_cursors, 16) != hipSuccess ||
        hipMemset(c->d_cursors, 0, 16 * sizeof(unsigned long long)) != hipSuccess ||
        c->h_overflow.grow(1) != hipSuccess ||
        c->pass_ev[0].create() != hipSuccess || c->pass_ev[1].create() != hipSuccess)
        return fail("ctl_create: cursor/event allocation failed");
    {
        std::vector<uint32_t> pw((size_t)kJumpBits * 800 + 130 * 800);
        ctl::sampler_step_powers(pw.data(), kJumpBits);
        ctl::sampler_seq_powers(pw.data() + kSeqPowBase, c->len);
        if (c->fixed.alloc(&c->d_powers, pw.size()) != hipSuccess ||
            hipMemcpy(c->d_powers, pw.data(), pw.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
            return fail("ctl_create: sampler power table allocation failed");
    }
    for (int i = 0; i < 2; i++) {
        size_t n1 = (size_t)c->nseq * c->len;
        if (c->fixed.alloc(&c->d_s1[i], n1) != hipSuccess || c->fixed.alloc(&c->d_s2[i], n1) != hipSuccess ||
            c->h_s1[i].grow(n1) != hipSuccess || c->h_s2[i].grow(n1 * 2) != hipSuccess ||
            c->ev[i].create(hipEventDisableTiming) != hipSuccess)
            return fail("ctl_create: sampler buffer allocation failed");
    }
    return c;
}

// The context's own buffers and events go with their owners (devmem.h).
CTL_API void ctl_destroy(ctl_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    free_scene(c);
    ctl::wpt_free(c);
    ctl::anim_free(c);
    ctl::image_free(c);
    delete c;
}

CTL_API ctl_status ctl_sampler_upload(ctl_ctx* c, const float* seq1d, const float* seq2d, uint32_t nseq, uint32_t len,
                                      void* stream) {
    if (!c || !seq1d || !seq2d) return CTL_ERR_INVALID;
    if (nseq != c->nseq || len != c->len) { c->err = "sampler_upload: tables must be 4096 x 30"; return CTL_ERR_INVALID; }
    CTL_HIP(c, hipSetDevice(c->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int b = c->next_buf;
    size_t n1 = (size_t)nseq * len;
    CTL_HIP(c, hipEventSynchronize(c->ev[b]));
    std::memcpy(c->h_s1[b].get(), seq1d, n1 * sizeof(float));
    std::memcpy(c->h_s2[b].get(), seq2d, n1 * 2 * sizeof(float));
    CTL_HIP(c, hipMemcpyAsync(c->d_s1[b], c->h_s1[b].get(), n1 * sizeof(float), hipMemcpyHostToDevice, s));
    CTL_HIP(c, hipMemcpyAsync(c->d_s2[b], c->h_s2[b].get(), n1 * 2 * sizeof(float), hipMemcpyHostToDevice, s));
    CTL_HIP(c, hipEventRecord(c->ev[b], s));
    c->active = b;
    c->next_buf = 1 - b;
    c->tables_pass = -1;   // caller's tables: no pass index to render ahead from
    c->scene_epoch++;
    return CTL_OK;
}

CTL_API ctl_status ctl_sampler_generate(ctl_ctx* c, uint64_t pass_index, void* stream) {
    // Generated on the device (sampler_kernel); stream order makes the buffer
    // reuse safe: the pass that read buffer b two calls ago precedes this launch.
    if (!c) return CTL_ERR_INVALID;
    CTL_HIP(c, hipSetDevice(c->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int b = c->next_buf;
    XorwowDev base;
    ctl::sampler_pass_state(pass_index, c->nseq, c->len, base.v, &base.d);
    hipLaunchKernelGGL(sampler_kernel, dim3((c->nseq + 3) / 4), dim3(256), 0, s, c->d_powers, base, c->nseq,
                       c->len, c->d_s1[b], c->d_s2[b]);
    CTL_HIP(c, hipGetLastError());
    c->active = b;
    c->next_buf = 1 - b;
    c->tables_pass = (int64_t)std::min<uint64_t>(pass_index, (uint64_t)INT64_MAX - 16);
    return CTL_OK;
}

// dcount != NULL: n and n2 are upper bounds (grid sizing); the kernel reads the
// segment sizes from dcount[0..1] on the device.
static ctl_status launch_intersect(ctl_ctx* c, int64_t n, const ctl_ray* rays, ctl_hit* hits, int32_t any_hit,
                                   bool stats, void* stream, int64_t n2 = 0, const ctl_ray* rays2 = nullptr,
                                   ctl_hit* hits2 = nullptr, const uint32_t* dcount = nullptr, uint32_t band_w = 0) {
    if (!c || n < 0 || (n > 0 && (!rays || !hits)) || n2 < 0 || (n2 > 0 && (!rays2 || !hits2))) return CTL_ERR_INVALID;
    if (!c->has_scene) { c->err = "intersect: no scene uploaded"; return CTL_ERR_STATE; }
    if (c->overflow_seen) return CTL_ERR_STATE;   // c->err names the overflow (ctl_sync)
    if (n + n2 > 0xffffffffll) { c->err = "intersect: more than 2^32-1 rays per call"; return CTL_ERR_INVALID; }
    CTL_HIP(c, hipSetDevice(c->device));
    if (n + n2 == 0) return CTL_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    unsigned long long* cursor = c->d_cursors;
    CTL_HIP(c, hipMemsetAsync(cursor, 0, sizeof(unsigned long long), s));
    const uint64_t want = ((uint64_t)(n + n2) + kBlock - 1) / kBlock;
#ifndef CTL_INTERSECT_BPC
#define CTL_INTERSECT_BPC 3   // resident blocks per CU of the batch traversal (0: occupancy limit)
#endif
    with_tree(stats, c->scene.single != 0, c->scene.wide != 0, [&](auto ST, auto SG, auto WD) {
        auto launch = [&](auto AN) {
            auto k = intersect_kernel<decltype(AN)::value, decltype(ST)::value, decltype(SG)::value,
                                      decltype(WD)::value>;
            hipLaunchKernelGGL(k, resident_grid(c, k, kStackLdsBytes, want, CTL_INTERSECT_BPC), dim3(kBlock),
                               kStackLdsBytes, s, c->scene, n, rays, hits, n2, rays2, hits2, cursor, c->d_counters,
                               dcount, band_w);
        };
        // 2 is internal: the WavefrontPathTracer's shadow query segment; a stats launch counts it as any-hit
        if (any_hit == 2 && !decltype(ST)::value) launch(std::integral_constant<int, 2>{});
        else if (any_hit) launch(std::integral_constant<int, 1>{});
        else launch(std::integral_constant<int, 0>{});
    });
    CTL_HIP(c, hipGetLastError());
    return CTL_OK;
}

static ctl_status add_rays(ctl_ctx* c, uint64_t n, hipStream_t s);

CTL_API ctl_status ctl_intersect(ctl_ctx* c, int64_t n, const ctl_ray* d_rays, ctl_hit* d_hits, int32_t any_hit,
                                 void* stream) {
    ctl_status r = launch_intersect(c, n, d_rays, d_hits, any_hit ? 1 : 0, false, stream);
    if (r != CTL_OK) return r;
    // the batch call counts N rays (g_RayTracedCounterHost += N, TraceHelper.cu:745)
    return add_rays(c, (uint64_t)n, reinterpret_cast<hipStream_t>(stream));
}

CTL_API ctl_status ctl_occluded(ctl_ctx* c, int64_t n, const ctl_ray* d_rays, uint32_t* d_out, int32_t any_hit,
                                void* stream) {
    if (!c || n < 0 || (n > 0 && (!d_rays || !d_out))) return CTL_ERR_INVALID;
    if (!c->has_scene) { c->err = "occluded: no scene uploaded"; return CTL_ERR_STATE; }
    if (c->overflow_seen) return CTL_ERR_STATE;   // c->err names the overflow (ctl_sync)
    CTL_HIP(c, hipSetDevice(c->device));
    if (n == 0) return CTL_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((n + kBlock - 1) / kBlock));
    if (grid.x == 0 || (uint64_t)(n + kBlock - 1) / kBlock > 0x7fffffffull) {
        c->err = "occluded: batch too large for one launch";
        return CTL_ERR_INVALID;
    }
    with_tree(c->scene.single != 0, c->scene.wide != 0, [&](auto SG, auto WD) {
        auto launch = [&](auto AQ) {
            hipLaunchKernelGGL((occluded_kernel<decltype(AQ)::value, decltype(SG)::value, decltype(WD)::value>), grid,
                               dim3(kBlock), kStackLdsBytes, s, c->scene, n, d_rays, d_out, c->d_counters);
        };
        if (any_hit) launch(std::true_type{}); else launch(std::false_type{});
    });
    CTL_HIP(c, hipGetLastError());
    return add_rays(c, (uint64_t)n, s);   // each Occluded is one traceRay (TraceHelper.cu:176)
}

static ctl_status prepare_pass(ctl_ctx* c, const ctl_pt_params* p, ctl_pixel* fb, PathParams& P,
                               bool need_tables = true) {
    if (!c || !p || !fb) return CTL_ERR_INVALID;
    if (!c->has_scene) { c->err = "render_pass: no scene uploaded"; return CTL_ERR_STATE; }
    if (c->overflow_seen) return CTL_ERR_STATE;   // c->err names the overflow (ctl_sync)
    if (need_tables && c->active < 0) {
        c->err = "render_pass: no sampler tables (call ctl_sampler_generate)";
        return CTL_ERR_STATE;
    }
    uint32_t ts = p->tile_size ? p->tile_size : 64;
    if (ts % 8 != 0) { c->err = "render_pass: tile_size must be a multiple of 8"; return CTL_ERR_INVALID; }
    uint32_t nr = p->num_ranks ? p->num_ranks : 1;
    if (p->rank >= nr) { c->err = "render_pass: rank >= num_ranks"; return CTL_ERR_INVALID; }
    const ctl_camera& cam = c->scene.camera;
    P.width = cam.width; P.height = cam.height;
    P.max_path_length = p->max_path_length;
    P.rr_start_depth = p->rr_start_depth;
    P.tile_size = ts;
    P.tiles_x = (cam.width + ts - 1) / ts;
    uint32_t tiles_y = (cam.height + ts - 1) / ts;
    P.num_tiles = P.tiles_x * tiles_y;
    P.num_ranks = nr;
    P.rank = p->rank;
    P.nseq = c->nseq; P.len = c->len;
    P.shadow_any_hit = p->shadow_any_hit;
    P.direct = p->direct != 0;
    P.half_quirk = c->half_quirk;
    P.owned_items = 0;
    P.apron = nr > 1 ? 2 * ts + 1 : 0;
    const uint64_t own = (uint64_t)owned_tiles_of(P) * ts * ts;
    if (own + (uint64_t)owned_tiles_of(P) * P.apron >= 0xffffffffull) {
        c->err = "render_pass: 2^32-1 or more work items per pass";
        return CTL_ERR_INVALID;
    }
    P.owned_items = (uint32_t)own;
    return CTL_OK;
}

static ctl_status launch_schedule(ctl_ctx* c, const ctl_pt_params* p, const PathParams& P, ctl_pixel* fb, bool stats,
                                  hipStream_t s, uint64_t threads, dim3 grid, const float* s1, const float2* s2,
                                  SampleSlots PS = make_slots(nullptr, 0), uint32_t tbl = 0);

static ctl_status prepare_slots(ctl_ctx* c, uint64_t items, hipStream_t s);
static void launch_fold(ctl_ctx* c, const PathParams& P, uint32_t per_pass, uint32_t n, ctl_pixel* fb, hipStream_t s,
                        uint32_t first_slice);

static ctl_status launch_pass(ctl_ctx* c, const ctl_pt_params* p, ctl_pixel* fb, bool stats, void* stream) {
    PathParams P;
    ctl_status r = prepare_pass(c, p, fb, P);
    if (r != CTL_OK) return r;
    CTL_HIP(c, hipSetDevice(c->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const uint64_t threads = pass_items_of(P);   // owned pixels + apron items
    if (threads == 0) return CTL_OK;
    dim3 grid((unsigned)((threads + kBlock - 1) / kBlock));
    const float* s1 = c->d_s1[c->active];
    const float2* s2 = c->d_s2[c->active];
    CTL_HIP(c, hipEventRecord(c->pass_ev[0], s));
    ctl_status r1 = prepare_slots(c, threads, s);   // every schedule stores samples per work item
    if (r1 != CTL_OK) return r1;
    ctl_status r2 = launch_schedule(c, p, P, fb, stats, s, threads, grid, s1, s2,
                                    make_slots(c->d_slices.get(), (uint32_t)threads), 0);
    if (r2 != CTL_OK) return r2;
    launch_fold(c, P, (uint32_t)threads, 1, fb, s, 0);
    CTL_HIP(c, hipEventRecord(c->pass_ev[1], s));
    c->pass_timed = true;
    return CTL_OK;
}

static ctl_status launch_schedule(ctl_ctx* c, const ctl_pt_params* p, const PathParams& P, ctl_pixel* fb, bool stats,
                                  hipStream_t s, uint64_t threads, dim3 grid, const float* s1, const float2* s2,
                                  SampleSlots PS, uint32_t tbl) {
    if (p->flags & CTL_PT_WAVEFRONT) return (ctl_status)ctl::wavefront_pass(c, P, PS, stats, s);
    const bool persistent = !(p->flags & CTL_PT_MEGAKERNEL);
    unsigned long long* cursor = c->d_cursors + 1;
    if (persistent) CTL_HIP(c, hipMemsetAsync(cursor, 0, sizeof(unsigned long long), s));
    const uint64_t want = (threads + kBlock - 1) / kBlock;
    const bool known = launch_path<CTL_PATH_LEVELS_HERE>(c, persistent, stats, P, s1, s2, threads, want, grid, cursor, fb,
                                                         PS, tbl, s) ||
                       ctl::media_launch_path(c, persistent, stats, P, s1, s2, threads, want, grid, cursor, fb, PS, tbl, s) ||
                       ctl::sensors_launch_path(c, persistent, stats, P, s1, s2, threads, want, grid, cursor, fb, PS, tbl, s);
    assert(known);
    (void)known;
    CTL_HIP(c, hipGetLastError());
    return CTL_OK;
}

// Sample slots -> framebuffer: per target pixel, the samples that landed on it
// (its own and the ones that rounded over from the left / upper / upper-left
// neighbour) in image order of their pixels, pass by pass -- one sequential
// AddSample per pixel in image order (Image.cu:22-44), as the oracle adds them.
// Only this rank's pixels are targets; a source of another rank is read from
// the target tile's apron item (source_item), so each pixel is summed by one
// rank in the 1-GPU order and the N-rank reduce is exact.
__global__ __launch_bounds__(kBlock) void fold_samples_kernel(PathParams P, const float4* __restrict__ slots,
                                                              uint32_t per_pass, uint32_t n, ctl_pixel* fb) {
    const uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= (uint64_t)P.width * P.height) return;
    const uint32_t x = (uint32_t)(q % P.width), y = (uint32_t)(q / P.width);
    const uint32_t ts = P.tile_size;
    if (((y / ts) * P.tiles_x + x / ts) % P.num_ranks != P.rank) return;   // the owner sums it (apron items)
    const uint32_t x0 = x - x % ts, y0 = y - y % ts;
    uint32_t ks[4];
    float codes[4];
    int nc = 0;
    // sources in image order: (x-1, y-1), (x, y-1), (x-1, y), (x, y)
#pragma unroll
    for (int d = 3; d >= 0; d--) {
        const uint32_t dx = d & 1, dy = d >> 1;
        uint32_t k;
        if (x >= dx && y >= dy && source_item(P, x - dx, y - dy, x0, y0, k)) {
            ks[nc] = k;
            codes[nc] = (float)(1 + d);
            nc++;
        }
    }
    if (nc == 0) return;
    ctl_pixel* pp = fb + q;
    float r = 0.0f, g = 0.0f, b = 0.0f, w = 0.0f;
    bool any = false;
    for (uint32_t k = 0; k < n; k++) {
        for (int i = 0; i < nc; i++) {
            const float4 v = slots[(size_t)k * per_pass + ks[i]];
            if (v.w == codes[i]) {
                if (!any) { r = pp->rgb[0]; g = pp->rgb[1]; b = pp->rgb[2]; w = pp->weight_sum; any = true; }
                r += v.x; g += v.y; b += v.z; w += 1.0f;
            }
        }
    }
    if (any) {
        pp->rgb[0] = r; pp->rgb[1] = g; pp->rgb[2] = b;
        pp->weight_sum = w;
    }
}

// Sample slots for n passes of per_pass work items, grown on demand.  Every
// work item writes its slot (code 0 when it has no pixel or AddSample would
// drop the sample), so no clearing is needed.
static ctl_status prepare_slots(ctl_ctx* c, uint64_t items, hipStream_t s) {
    c->spec.pending = false;   // the slots are about to be overwritten
    if (!c->d_slices.fits(items)) {
        CTL_HIP(c, hipStreamSynchronize(s));
        if (c->d_slices.grow(items) != hipSuccess) {
            c->err = "render_pass: sample slot allocation failed";
            return CTL_ERR_NOMEM;
        }
    }
    return CTL_OK;
}

static void launch_fold(ctl_ctx* c, const PathParams& P, uint32_t per_pass, uint32_t n, ctl_pixel* fb, hipStream_t s,
                        uint32_t first_slice = 0) {
    const uint64_t px = (uint64_t)P.width * P.height;
    hipLaunchKernelGGL(fold_samples_kernel, dim3((unsigned)((px + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, P,
                       c->d_slices.get() + (size_t)first_slice * per_pass, per_pass, n, fb);
}

// n_passes consecutive passes in one persistent launch; the first n_fold of them
// are folded into d_fb, the rest stay in the sample slots (a speculative window).
static ctl_status launch_window(ctl_ctx* c, const ctl_pt_params* params, uint64_t first_pass, uint32_t n_passes,
                                uint32_t n_fold, ctl_pixel* d_fb, hipStream_t s, uint64_t* per_pass_out);

CTL_API ctl_status ctl_render_passes(ctl_ctx* c, const ctl_pt_params* params, uint64_t first_pass, uint32_t n_passes,
                                     ctl_pixel* d_fb, void* stream) {
    if (!c || !params || !d_fb) return CTL_ERR_INVALID;
    if (n_passes == 0) return CTL_OK;
    c->spec.last_valid = false;
    return launch_window(c, params, first_pass, n_passes, n_passes, d_fb, reinterpret_cast<hipStream_t>(stream), nullptr);
}

static ctl_status launch_window(ctl_ctx* c, const ctl_pt_params* params, uint64_t first_pass, uint32_t n_passes,
                                uint32_t n_fold, ctl_pixel* d_fb, hipStream_t s, uint64_t* per_pass_out) {
    void* stream = reinterpret_cast<void*>(s);
    if (params->flags & (CTL_PT_WAVEFRONT | CTL_PT_MEGAKERNEL)) {
        // the other schedules: one pass at a time
        for (uint32_t i = 0; i < n_passes; i++) {
            ctl_status r = ctl_sampler_generate(c, first_pass + i, stream);
            if (r == CTL_OK) r = launch_pass(c, params, d_fb, false, stream);
            if (r != CTL_OK) return r;
        }
        return CTL_OK;
    }
    PathParams P;
    ctl_status r = prepare_pass(c, params, d_fb, P, false);
    if (r != CTL_OK) return r;
    CTL_HIP(c, hipSetDevice(c->device));
    const uint64_t per_pass = pass_items_of(P);   // owned pixels + apron items
    if (per_pass_out) *per_pass_out = per_pass;
    if (per_pass == 0) return CTL_OK;
    const uint64_t items = per_pass * n_passes;
    if (items >= 0xffffffffull) { c->err = "render_passes: 2^32-1 or more work items"; return CTL_ERR_INVALID; }
    const size_t tbl = (size_t)c->nseq * c->len;
    if (!c->d_mt1.fits(tbl * n_passes) || !c->d_mt2.fits(tbl * n_passes)) {
        CTL_HIP(c, hipStreamSynchronize(s));
        c->d_mt1.reset();
        c->d_mt2.reset();
        if (c->d_mt1.grow(tbl * n_passes) != hipSuccess || c->d_mt2.grow(tbl * n_passes) != hipSuccess) {
            c->err = "render_passes: sampler table allocation failed";
            return CTL_ERR_NOMEM;
        }
    }
    CTL_HIP(c, hipEventRecord(c->pass_ev[0], s));
    for (uint32_t i0 = 0; i0 < n_passes; i0 += kSamplerBatch) {
        const uint32_t nb = std::min(kSamplerBatch, n_passes - i0);
        SamplerBases B;
        for (uint32_t i = 0; i < nb; i++)
            ctl::sampler_pass_state(first_pass + i0 + i, c->nseq, c->len, B.b[i].v, &B.b[i].d);
        hipLaunchKernelGGL(sampler_batch_kernel, dim3((c->nseq + 3) / 4, nb), dim3(256), 0, s, c->d_powers, B, c->nseq,
                           c->len, c->d_mt1.get() + i0 * tbl, c->d_mt2.get() + i0 * tbl, (uint64_t)tbl);
    }
    r = prepare_slots(c, items, s);
    if (r != CTL_OK) return r;
    r = launch_schedule(c, params, P, d_fb, false, s, items, dim3(1), c->d_mt1.get(), c->d_mt2.get(),
                        make_slots(c->d_slices.get(), (uint32_t)per_pass), (uint32_t)tbl);
    if (r != CTL_OK) return r;
    launch_fold(c, P, (uint32_t)per_pass, n_fold, d_fb, s, 0);
    CTL_HIP(c, hipGetLastError());
    CTL_HIP(c, hipEventRecord(c->pass_ev[1], s));
    c->pass_timed = true;
    return CTL_OK;
}

// Tracer::DoPass through the C ABI with CTL_PT_RENDER_AHEAD (see ctl_ctx::Spec):
// a call whose pass was rendered ahead by an earlier call of the same window
// only folds its samples; a call that continues a steady loop renders a window
// of 2, 4, then 8 passes and folds the first.  Bit-exact to one launch per pass (the fold adds pass by
// pass in the same order); ctl_rays_traced counts a window's rays when it is
// launched, ctl_last_pass_ms times the call's own device work.
static ctl_status render_pass_speculative(ctl_ctx* c, const ctl_pt_params* params, ctl_pixel* d_fb, void* stream) {
    if (!c || !params || !d_fb) return CTL_ERR_INVALID;
    ctl_ctx::Spec& W = c->spec;
    const bool same_state = W.last_valid && std::memcmp(&W.params, params, sizeof(ctl_pt_params)) == 0 && W.fb == d_fb &&
                            W.stream == stream && W.epoch == c->scene_epoch && c->tables_pass >= 0;
    const bool next_pass = same_state && c->tables_pass == W.last_pass + 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (W.pending && next_pass && c->tables_pass == W.next && !c->overflow_seen) {
        // rendered ahead: fold its slice
        PathParams P;
        ctl_status r = prepare_pass(c, params, d_fb, P);
        if (r != CTL_OK) return r;
        CTL_HIP(c, hipSetDevice(c->device));
        CTL_HIP(c, hipEventRecord(c->pass_ev[0], s));
        launch_fold(c, P, (uint32_t)W.per_pass, 1, d_fb, s, (uint32_t)(W.next - W.first));
        CTL_HIP(c, hipGetLastError());
        CTL_HIP(c, hipEventRecord(c->pass_ev[1], s));
        c->pass_timed = true;
        W.last_pass = W.next++;
        if (W.next == W.end) { W.pending = false; W.streak++; }
        return CTL_OK;
    }
    if (W.pending) W.streak = 0;   // the loop left the window: its passes are dropped
    W.pending = false;
    const bool speculate = next_pass && (params->flags & CTL_PT_RENDER_AHEAD) &&
                           !(params->flags & (CTL_PT_WAVEFRONT | CTL_PT_MEGAKERNEL));
    if (!speculate) W.streak = 0;
    const uint32_t n = speculate ? (W.streak >= 2 ? 8u : W.streak == 1 ? 4u : 2u) : 1u;
    ctl_status r;
    uint64_t per_pass = 0;
    if (n == 1) {
        r = launch_pass(c, params, d_fb, false, stream);
    } else {
        PathParams P;
        r = prepare_pass(c, params, d_fb, P);   // the tables of this pass are there; refusals as launch_pass's
        if (r == CTL_OK) r = launch_window(c, params, (uint64_t)c->tables_pass, n, 1, d_fb, s, &per_pass);
    }
    if (r != CTL_OK) { W.last_valid = false; return r; }
    W.last_valid = c->tables_pass >= 0;
    W.last_pass = c->tables_pass;
    W.params = *params;
    W.fb = d_fb;
    W.stream = stream;
    W.epoch = c->scene_epoch;
    if (n > 1 && per_pass > 0) {
        W.pending = true;
        W.per_pass = per_pass;
        W.first = c->tables_pass;
        W.next = c->tables_pass + 1;
        W.end = c->tables_pass + n;
    }
    return CTL_OK;
}

CTL_API ctl_status ctl_render_pass(ctl_ctx* c, const ctl_pt_params* params, ctl_pixel* d_fb, void* stream) {
#ifdef CTL_PROFILE_TRACE
    ctl_status r = launch_pass(c, params, d_fb, false, stream);
    unsigned long long v[11];
    if (hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)) == hipSuccess &&
        hipMemcpy(v, c->d_counters + 5, sizeof(v), hipMemcpyDeviceToHost) == hipSuccess) {
        fprintf(stderr, "[profile] trace/total wave time %.4f (%llu / %llu); inner loop: %llu wave iterations, "
                        "%.1f lanes each; leaf entries: %llu wave iterations, %.1f lanes each\n",
                (double)v[0] / (double)v[1], v[0], v[1], v[4], (double)v[3] / (double)v[4], v[6],
                (double)v[5] / (double)v[6]);
        fprintf(stderr, "[profile] lanes in the round per inner iteration %.1f; rounds %llu, lanes holding a leaf at the "
                        "leaf phase %.1f\n", (double)v[7] / (double)v[4], v[8], (double)v[9] / (double)v[8]);
        fprintf(stderr, "[profile] tail hand-over: %llu lanes handed over at %llu breaks of the trace loop\n",
                v[kTailHandovers - 5], v[kTailBreaks - 5]);
        (void)hipMemset(c->d_counters + 5, 0, sizeof(v));
    }
    return r;
#else
    return render_pass_speculative(c, params, d_fb, stream);
#endif
}

// fold_samples_kernel of a block-list pass: one thread per pixel of a listed
// block (slot-major, row-major inside the block), so only listed blocks are
// visited.  The pixel's sources are added in image order, and that m times in
// succession for a block listed m times -- what m full passes add to it.
__global__ __launch_bounds__(kBlock) void fold_blocks_kernel(PathParams P, const uint32_t* __restrict__ T,
                                                             const float4* __restrict__ slots, ctl_pixel* fb) {
    const uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= P.owned_items) return;
    const uint32_t ts = P.tile_size, perTile = ts * ts;
    const uint32_t slot = (uint32_t)(q / perTile), w = (uint32_t)(q % perTile);
    const uint32_t m = T[OwnList::mult_off(P.num_tiles) + slot];
    const uint2 o = OwnList::origin(T, slot);
    const uint32_t x0 = o.x, y0 = o.y;
    const uint32_t x = x0 + w % ts, y = y0 + w / ts;
    if (x >= P.width || y >= P.height) return;
    // sources in image order: (x-1, y-1), (x, y-1), (x-1, y), (x, y); v[i] and
    // has[i] are indexed by unrolled constants only, so they stay in registers
    float4 v[4];
    bool has[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int d = 3 - i;
        const uint32_t dx = d & 1, dy = d >> 1;
        has[i] = false;
        if (x >= dx && y >= dy) {
            v[i] = slots[OwnList::source_item(P, T, x - dx, y - dy, slot, x0, y0)];
            has[i] = v[i].w == (float)(1 + d);
        }
    }
    if (!(has[0] || has[1] || has[2] || has[3])) return;
    ctl_pixel* pp = fb + (size_t)y * P.width + x;
    float r = pp->rgb[0], g = pp->rgb[1], b = pp->rgb[2], ws = pp->weight_sum;
    for (uint32_t k = 0; k < m; k++) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (has[i]) { r += v[i].x; g += v[i].y; b += v[i].z; ws += 1.0f; }
        }
    }
    pp->rgb[0] = r; pp->rgb[1] = g; pp->rgb[2] = b;
    pp->weight_sum = ws;
}

static const char* schedule_name(uint32_t flags) {
    return (flags & CTL_PT_WAVEFRONT) ? "CTL_PT_WAVEFRONT" : "CTL_PT_MEGAKERNEL";
}

CTL_API ctl_status ctl_render_pass_blocks(ctl_ctx* c, const ctl_pt_params* p, const uint32_t* blocks, uint32_t n_blocks,
                                          ctl_pixel* d_fb, void* stream) {
    if (!c || !p || !d_fb || (!blocks && n_blocks)) return CTL_ERR_INVALID;
    if (p->flags & (CTL_PT_WAVEFRONT | CTL_PT_MEGAKERNEL)) {
        c->err = std::string("render_pass_blocks: block lists run in the persistent schedule only, not ") +
                 schedule_name(p->flags);
        return CTL_ERR_INVALID;
    }
    if (p->num_ranks > 1) { c->err = "render_pass_blocks: num_ranks must be 1"; return CTL_ERR_INVALID; }
    PathParams P;
    ctl_status r = prepare_pass(c, p, d_fb, P);
    if (r != CTL_OK) return r;
    c->spec.pending = false;   // a render-ahead window does not survive a block-list pass
    c->spec.last_valid = false;
    c->spec.streak = 0;
    if (n_blocks == 0) return CTL_OK;
    CTL_HIP(c, hipSetDevice(c->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const uint32_t nt = P.num_tiles, ts = P.tile_size;
    if (!c->d_block_tbl.fits(OwnList::words(nt)) || !c->h_block_tbl.fits(2 * OwnList::words(nt))) {
        for (int i = 0; i < 2; i++) {
            if (c->block_ev_set[i]) CTL_HIP(c, hipEventSynchronize(c->block_ev[i]));
            c->block_ev_set[i] = false;
            if (!c->block_ev[i])
                CTL_HIP_AS(c, c->block_ev[i].create(hipEventDisableTiming), "hipEventCreateWithFlags");
        }
        CTL_HIP(c, hipStreamSynchronize(s));
        c->d_block_tbl.reset();
        c->h_block_tbl.reset();
        if (c->d_block_tbl.grow(OwnList::words(nt)) != hipSuccess ||
            c->h_block_tbl.grow(2 * OwnList::words(nt)) != hipSuccess) {
            c->err = "render_pass_blocks: block table allocation failed";
            return CTL_ERR_NOMEM;
        }
    }
    // the staging half of two calls ago: its upload has usually long left it
    const uint32_t half = c->block_half;
    if (c->block_ev_set[half]) CTL_HIP(c, hipEventSynchronize(c->block_ev[half]));
    // OwnList tables (common.h): slots in order of first appearance in the list
    uint32_t* origin = c->h_block_tbl.get() + half * c->d_block_tbl.cap();
    uint32_t* slot_of = origin + OwnList::slot_of_off(nt);
    uint32_t* mult = origin + OwnList::mult_off(nt);
    std::fill(origin, origin + 2 * (size_t)nt, 0u);
    std::fill(slot_of, slot_of + nt, kUnlisted);
    std::fill(mult, mult + nt, 0u);
    uint32_t n_slots = 0;
    for (uint32_t i = 0; i < n_blocks; i++) {
        const uint32_t b = blocks[i];
        if (b >= nt) {
            c->err = "render_pass_blocks: block id " + std::to_string(b) + " >= " + std::to_string(nt) + " blocks";
            return CTL_ERR_INVALID;
        }
        if (slot_of[b] == kUnlisted) {
            origin[2 * n_slots] = (b % P.tiles_x) * ts;
            origin[2 * n_slots + 1] = (b / P.tiles_x) * ts;
            slot_of[b] = n_slots++;
        }
        if (++mult[slot_of[b]] > 255) {
            c->err = "render_pass_blocks: block " + std::to_string(b) + " listed more than 255 times";
            return CTL_ERR_INVALID;
        }
    }
    P.apron = 2 * ts + 1;
    const uint64_t own = (uint64_t)n_slots * ts * ts, items = own + (uint64_t)n_slots * P.apron;
    if (items > kListItemMask) { c->err = "render_pass_blocks: 2^29 or more work items"; return CTL_ERR_INVALID; }
    P.owned_items = (uint32_t)own;
    CTL_HIP(c, hipEventRecord(c->pass_ev[0], s));
    CTL_HIP(c, hipMemcpyAsync(c->d_block_tbl.get(), origin, OwnList::words(nt) * sizeof(uint32_t), hipMemcpyHostToDevice,
                              s));
    CTL_HIP(c, hipEventRecord(c->block_ev[half], s));
    c->block_ev_set[half] = true;
    c->block_half = half ^ 1;
    r = prepare_slots(c, items, s);
    if (r != CTL_OK) return r;
    unsigned long long* cursor = c->d_cursors + 1;
    CTL_HIP(c, hipMemsetAsync(cursor, 0, sizeof(unsigned long long), s));
    const uint64_t want = (items + kBlock - 1) / kBlock;
    const SampleSlots PS = make_slots(c->d_slices.get(), (uint32_t)items);
    const float* s1 = c->d_s1[c->active];
    const float2* s2 = c->d_s2[c->active];
    const uint32_t* own_tbl = c->d_block_tbl.get();
    const bool known = launch_path_blocks<CTL_PATH_LEVELS_HERE>(c, P, s1, s2, items, want, cursor, PS, own_tbl, s) ||
                       ctl::media_launch_blocks(c, P, s1, s2, items, want, cursor, PS, own_tbl, s) ||
                       ctl::sensors_launch_blocks(c, P, s1, s2, items, want, cursor, PS, own_tbl, s);
    assert(known);
    (void)known;
    CTL_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(fold_blocks_kernel, dim3((unsigned)((own + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, P,
                       (const uint32_t*)c->d_block_tbl.get(), (const float4*)c->d_slices.get(), d_fb);
    CTL_HIP(c, hipGetLastError());
    CTL_HIP(c, hipEventRecord(c->pass_ev[1], s));
    c->pass_timed = true;
    return CTL_OK;
}

CTL_API ctl_status ctl_last_pass_ms(ctl_ctx* c, float* ms) {
    if (!c || !ms) return CTL_ERR_INVALID;
    if (!c->pass_timed) { c->err = "last_pass_ms: no render pass yet"; return CTL_ERR_STATE; }
    CTL_HIP(c, hipSetDevice(c->device));
    CTL_HIP(c, hipEventSynchronize(c->pass_ev[1]));
    CTL_HIP(c, hipEventElapsedTime(ms, c->pass_ev[0], c->pass_ev[1]));
    return CTL_OK;
}

CTL_API ctl_status ctl_camera_rays(ctl_ctx* c, const ctl_pt_params* params, ctl_ray* d_rays, int64_t capacity,
                                   int64_t* n_out, void* stream) {
    if (!c || !params || !n_out) return CTL_ERR_INVALID;
    PathParams P;
    ctl_pixel dummy;
    ctl_status r = prepare_pass(c, params, &dummy, P);
    if (r != CTL_OK) return r;
    const uint64_t items = P.owned_items;   // this rank's pixels
    *n_out = (int64_t)items;
    if (items == 0 || !d_rays) return CTL_OK;   // d_rays == NULL: size query
    if (capacity < (int64_t)items) { c->err = "camera_rays: ray buffer too small"; return CTL_ERR_INVALID; }
    CTL_HIP(c, hipSetDevice(c->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // a scene seen through another sensor than the perspective one: that level's kernel (path_sensors.hip)
    if (!ctl::sensors_launch_camera_rays(c, P, c->d_s1[c->active], c->d_s2[c->active], items, d_rays, s))
        hipLaunchKernelGGL(camera_ray_kernel, dim3((unsigned)((items + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                           c->scene, P, c->d_s1[c->active], c->d_s2[c->active], items, d_rays);
    CTL_HIP(c, hipGetLastError());
    return CTL_OK;
}

__global__ void add_kernel(unsigned long long* ctr, unsigned long long k) { ctr[0] += k; }

static ctl_status add_rays(ctl_ctx* c, uint64_t n, hipStream_t s) {
    hipLaunchKernelGGL(add_kernel, dim3(1), dim3(1), 0, s, c->d_counters, (unsigned long long)n);
    CTL_HIP(c, hipGetLastError());
    return CTL_OK;
}

}  // extern "C"

namespace ctl {
int intersect_launch(ctl_ctx* c, int64_t n, const ctl_ray* rays, ctl_hit* hits, int32_t any_hit, hipStream_t s,
                     int64_t n2, const ctl_ray* rays2, ctl_hit* hits2, const uint32_t* dcount, uint32_t band_w) {
    return launch_intersect(c, n, rays, hits, any_hit, false, s, n2, rays2, hits2, dcount, band_w);
}
int count_rays(ctl_ctx* c, uint64_t n, hipStream_t s) { return add_rays(c, n, s); }
}  // namespace ctl

extern "C" {

static void note_overflow(ctl_ctx* c, unsigned long long lanes) {
    if (!lanes) return;
    c->overflow_seen = true;
    c->err = "traversal stack overflow on " + std::to_string(lanes) + " lanes (results invalid; ctl_reset_rays clears)";
}

CTL_API uint64_t ctl_rays_traced(ctl_ctx* c) {
    if (!c) return 0;
    unsigned long long v[2] = {0, 0};
    if (hipSetDevice(c->device) != hipSuccess) return 0;
    if (hipDeviceSynchronize() != hipSuccess) return 0;
    if (hipMemcpy(v, c->d_counters, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return 0;
    note_overflow(c, v[1]);
    return v[0];
}

CTL_API ctl_status ctl_tail_handovers(ctl_ctx* c, uint64_t* lanes, uint64_t* breaks) {
    if (!c) return CTL_ERR_INVALID;
    unsigned long long v[16];
    CTL_HIP(c, hipSetDevice(c->device));
    CTL_HIP(c, hipDeviceSynchronize());
    CTL_HIP(c, hipMemcpy(v, c->d_counters, sizeof(v), hipMemcpyDeviceToHost));
    if (lanes) *lanes = v[kTailHandovers];
    if (breaks) *breaks = v[kTailBreaks];
    return CTL_OK;
}

CTL_API int32_t ctl_scene_stack_bound(const ctl_ctx* c) { return c && c->has_scene ? c->stack_bound : 0; }

CTL_API ctl_status ctl_reset_rays(ctl_ctx* c, void* stream) {
    if (!c) return CTL_ERR_INVALID;
    CTL_HIP(c, hipSetDevice(c->device));
    CTL_HIP(c, hipMemsetAsync(c->d_counters, 0, 16 * sizeof(unsigned long long), reinterpret_cast<hipStream_t>(stream)));
    c->overflow_seen = false;
    return CTL_OK;
}

// The sync point of the C ABI: waits for the stream, then reports a traversal
// stack overflow of any earlier launch as CTL_ERR_STATE (sticky until
// ctl_reset_rays; every later render / intersect call refuses to run).
CTL_API ctl_status ctl_sync(ctl_ctx* c, void* stream) {
    if (!c) return CTL_ERR_INVALID;
    CTL_HIP(c, hipSetDevice(c->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    CTL_HIP(c, hipMemcpyAsync(c->h_overflow.get(), c->d_counters + 1, sizeof(unsigned long long), hipMemcpyDeviceToHost,
                              s));
    CTL_HIP(c, hipStreamSynchronize(s));
    note_overflow(c, *c->h_overflow.get());
    return c->overflow_seen ? CTL_ERR_STATE : CTL_OK;
}

static ctl_status read_stats(ctl_ctx* c, uint64_t out[4], uint64_t rays_before, hipStream_t s) {
    unsigned long long v[5];
    CTL_HIP(c, hipStreamSynchronize(s));
    CTL_HIP(c, hipMemcpy(v, c->d_counters, sizeof(v), hipMemcpyDeviceToHost));
    out[0] = v[0] - rays_before;
    out[1] = v[2]; out[2] = v[3]; out[3] = v[4];
    CTL_HIP(c, hipMemset(c->d_counters + 2, 0, 3 * sizeof(unsigned long long)));
    note_overflow(c, v[1]);
    if (c->overflow_seen) return CTL_ERR_STATE;
    return CTL_OK;
}

// Opens a stats call: waits for the stream, clears the statistics counters
// [2..4] and reads the ray count the call starts from (read_stats closes it).
static ctl_status begin_stats(ctl_ctx* c, unsigned long long& before, hipStream_t s) {
    CTL_HIP(c, hipStreamSynchronize(s));
    CTL_HIP(c, hipMemset(c->d_counters + 2, 0, 3 * sizeof(unsigned long long)));
    CTL_HIP(c, hipMemcpy(&before, c->d_counters, sizeof(before), hipMemcpyDeviceToHost));
    return CTL_OK;
}

CTL_API ctl_status ctl_intersect_stats(ctl_ctx* c, int64_t n, const ctl_ray* d_rays, ctl_hit* d_hits, int32_t any_hit,
                                       uint64_t out[4], void* stream) {
    if (!c || !out) return CTL_ERR_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    unsigned long long before = 0;
    ctl_status r = begin_stats(c, before, s);
    if (r != CTL_OK) return r;
    r = launch_intersect(c, n, d_rays, d_hits, any_hit ? 1 : 0, true, stream);
    if (r != CTL_OK) return r;
    if ((r = add_rays(c, (uint64_t)n, s)) != CTL_OK) return r;
    return read_stats(c, out, before, s);
}

CTL_API ctl_status ctl_render_pass_stats(ctl_ctx* c, const ctl_pt_params* params, ctl_pixel* d_fb, uint64_t out[4],
                                         void* stream) {
    if (!c || !out) return CTL_ERR_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    unsigned long long before = 0;
    ctl_status r = begin_stats(c, before, s);
    if (r != CTL_OK) return r;
    r = launch_pass(c, params, d_fb, true, stream);
    if (r != CTL_OK) return r;
    return read_stats(c, out, before, s);
}

}  // extern "C"
