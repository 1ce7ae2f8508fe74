// common.h — device pieces shared by the megakernel (ctl_trace.hip) and the
// wavefront pipeline (wavefront.hip): pass parameters, the SequenceSampler,
// sensor rays, AddSample, and the context structure of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cassert>
#include <string>
#include <vector>

#include "devmem.h"
#include "dispatch.h"
#include "traverse.h"
#include "../ctl_env.h"
#include "../ctl_light.h"
#include "../ctl_medium.h"
#include "../ctl_sensor.h"

namespace ctl {

constexpr int kBlock = 256;

struct PathParams {
    uint32_t width, height;
    int32_t max_path_length, rr_start_depth;
    uint32_t tile_size, tiles_x, num_tiles, num_ranks, rank;
    uint32_t nseq, len;
    int32_t shadow_any_hit;
    int32_t direct;   // KEY_Direct: PathTrace<true> (NEE + MIS) or PathTrace<false>
    bool half_quirk;
    // N > 1 ranks: work items [0, owned_items) are this rank's pixels; then, per
    // owned tile, apron (2 ts + 1 items: left column, top row, corner) -- the
    // other ranks' pixels whose jittered sample can land in the tile (ApronItem)
    uint32_t owned_items;
    uint32_t apron;   // 2 * tile_size + 1 when num_ranks > 1, else 0
};

// d1 / d2: the 1D / 2D draw counters reduced modulo len -- the reference only
// ever uses counter % len (the table row), and (d + 1) % len follows from
// d % len with a compare, so no division (and no loop-held reciprocal) per draw.
struct SamplerDev {   // SequenceSampler (Kernel/Sampler_device.h:59-113)
    const float* s1;
    const float2* s2;
    uint32_t nseq, len, a, b;   // a = idx % nseq, b = (idx / nseq) % nseq
    uint32_t d1, d2;            // draw counters mod len
    __device__ __forceinline__ void init(const float* t1, const float2* t2, uint32_t n, uint32_t l, uint32_t idx,
                                         uint32_t c1 = 0, uint32_t c2 = 0) {
        s1 = t1; s2 = t2; nseq = n; len = l;
        a = idx % n; b = (idx / n) % n;
        d1 = c1 % len; d2 = c2 % len;
    }
    __device__ __forceinline__ float next1() {
        const uint32_t k = d1;
        float val = 0.0f;
        val += s1[k * nseq + a];
        val += s1[k * nseq + b];
        d1 = d1 + 1 == len ? 0u : d1 + 1;
        return fracf_ref(val);
    }
    __device__ __forceinline__ f2 next2() {
        const uint32_t k = d2;
        float2 p = s2[k * nseq + a], q = s2[k * nseq + b];
        float x = 0.0f, y = 0.0f;
        x += p.x; y += p.y;
        x += q.x; y += q.y;
        d2 = d2 + 1 == len ? 0u : d2 + 1;
        return mk2(fracf_ref(x), fracf_ref(y));
    }
    // the value next2() returned as the sequence's 2-D draw number `draw`, whatever the counters are now
    __device__ __forceinline__ f2 peek2(uint32_t draw) const {
        const uint32_t k = draw % len;
        float2 p = s2[k * nseq + a], q = s2[k * nseq + b];
        float x = 0.0f, y = 0.0f;
        x += p.x; y += p.y;
        x += q.x; y += q.y;
        return mk2(fracf_ref(x), fracf_ref(y));
    }
};

struct LutDecode {
    const float4* lut;
    __device__ __forceinline__ f3 operator()(uint32_t c) const { float4 q = lut[c]; return mk3(q.x, q.y, q.z); }
};

__device__ __forceinline__ m44 load_m44(const float4* M) {
    float4 r0 = M[0], r1 = M[1], r2 = M[2], r3 = M[3];
    m44 m;
    m.d[0] = r0.x; m.d[1] = r0.y; m.d[2] = r0.z; m.d[3] = r0.w;
    m.d[4] = r1.x; m.d[5] = r1.y; m.d[6] = r1.z; m.d[7] = r1.w;
    m.d[8] = r2.x; m.d[9] = r2.y; m.d[10] = r2.z; m.d[11] = r2.w;
    m.d[12] = r3.x; m.d[13] = r3.y; m.d[14] = r3.z; m.d[15] = r3.w;
    return m;
}

// Number of set bits of `mask` below the calling lane (mbcnt: no per-lane
// mask register held for the kernel's lifetime).
__device__ __forceinline__ uint32_t lanes_below(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// The same pointer, opaque to the optimiser: reads through it (and the
// integer-division reciprocals of the fields read) stay where they are used
// instead of being hoisted out of a loop into registers held for its lifetime.
template <class T>
__device__ __forceinline__ const T* opaque_ptr(const T* p) {
    asm volatile("" : "+s"(p));
    return p;
}

__device__ __forceinline__ void wave_add_u64(unsigned long long* dst, uint64_t v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, (unsigned long long)v);
}

// Wave-aggregated claim: the lanes of `mask` (= __ballot(need), non-zero) take
// consecutive slots from *cursor with one atomic per wave; a claiming lane's slot.
template <class I>
__device__ __forceinline__ I wave_claim(I* cursor, uint64_t mask) {
    const int leader = __ffsll((unsigned long long)mask) - 1;
    I base = 0;
    if ((int)(threadIdx.x & 63) == leader) base = atomicAdd(cursor, (I)__popcll(mask));
    base = __shfl(base, leader);
    return base + (I)lanes_below(mask);
}

// Slots of ctl_ctx::d_counters (16 words) beside [0] rays, [1] overflow, [2..4] statistics and the
// CTL_PROFILE_TRACE build's [5], [6], [8..14]: the tail hand-over's lanes handed over and trace loops
// left early (persistent_loop.h; ctl_tail_handovers)
constexpr int kTailHandovers = 7, kTailBreaks = 15;

// End of a tracing kernel: the overflow flag and (STATS) the traversal statistics into counters[1..4]
template <bool STATS>
__device__ __forceinline__ void flush_counters(unsigned long long* counters, bool overflow, const TraceStats& ts) {
    if (overflow) atomicAdd(&counters[1], 1ull);
    if (STATS) {
        wave_add_u64(&counters[2], ts.nodes);
        wave_add_u64(&counters[3], ts.tris);
        wave_add_u64(&counters[4], ts.inst);
    }
}

// work item g -> pixel of the owned tiles (tile_id % num_ranks == rank); each
// wave covers an 8x8 pixel block so primary rays in a wave are coherent.
// Work items of one pass: the rank's pixels, then the apron items.
__host__ __device__ inline uint32_t owned_tiles_of(const PathParams& P) {
    return P.num_tiles > P.rank ? (P.num_tiles - P.rank + P.num_ranks - 1) / P.num_ranks : 0u;
}
__host__ __device__ inline uint64_t pass_items_of(const PathParams& P) {
    return (uint64_t)P.owned_items + (uint64_t)owned_tiles_of(P) * P.apron;
}

// Apron items (N > 1 ranks).  A sample lands on floor(pX): its own pixel or,
// when the jitter rounds up, the right / lower / lower-right neighbour, which
// may belong to another rank's tile.  So that every pixel's samples are summed
// by one rank in the 1-GPU order (fold_samples_kernel), the owner of the
// target tile traces such a foreign pixel's path itself: apron item (tile, i)
// is the pixel left of / above / above-left of the tile; it is traced only
// when its sample lands inside that tile (apron_keep), which needs just the
// first sampler draw, so the duplicated work is a few paths per image.
__device__ __forceinline__ bool apron_pixel(const PathParams& P, uint64_t a, uint32_t& px, uint32_t& py,
                                            uint32_t& x0, uint32_t& y0) {
    const uint32_t ts = P.tile_size;
    const uint32_t j = (uint32_t)(a / P.apron), i = (uint32_t)(a % P.apron);
    const uint32_t tile = j * P.num_ranks + P.rank;
    if (tile >= P.num_tiles) return false;
    x0 = (tile % P.tiles_x) * ts;
    y0 = (tile / P.tiles_x) * ts;
    if (i < ts) { if (x0 == 0) return false; px = x0 - 1; py = y0 + i; }
    else if (i < 2 * ts) { if (y0 == 0) return false; px = x0 + (i - ts); py = y0 - 1; }
    else { if (x0 == 0 || y0 == 0) return false; px = x0 - 1; py = y0 - 1; }
    if (px >= P.width || py >= P.height) return false;
    const uint32_t t2 = (py / ts) * P.tiles_x + px / ts;
    return t2 % P.num_ranks != P.rank;   // a pixel of this rank is covered by its own item
}

__device__ __forceinline__ bool work_pixel(const PathParams& P, uint64_t g, uint32_t& px, uint32_t& py) {
    if (P.apron && g >= P.owned_items) {
        uint32_t x0, y0;
        return apron_pixel(P, g - P.owned_items, px, py, x0, y0);
    }
    const uint32_t perTile = P.tile_size * P.tile_size;
    const uint32_t j = (uint32_t)(g / perTile), w = (uint32_t)(g % perTile);
    const uint32_t tile = j * P.num_ranks + P.rank;
    if (tile >= P.num_tiles) return false;
    const uint32_t groupsPerRow = P.tile_size / 8;
    const uint32_t grp = w / 64, lane = w % 64;
    px = (tile % P.tiles_x) * P.tile_size + (grp % groupsPerRow) * 8 + lane % 8;
    py = (tile / P.tiles_x) * P.tile_size + (grp / groupsPerRow) * 8 + lane / 8;
    return px < P.width && py < P.height;
}

// PerspectiveSensor::sampleRayDifferential (SceneTypes/Sensor.cu:130-144), primary ray only
__device__ __forceinline__ void sensor_ray(const DevScene& S, f2 pX, f3& o, f3& d) {
    m44 s2c = to_m44(S.camera.sample_to_camera), tw = to_m44(S.camera.to_world);
    f3 nearP = xform_point(s2c, mk3(pX.x * S.camera.inv_resolution[0], pX.y * S.camera.inv_resolution[1], 0.0f));
    f3 dd = normalize(nearP);
    o = xform_point(tw, mk3s(0.0f));
    d = xform_dir(tw, dd);
}

// Image::AddSample (Engine/Image.cu:22-44); one owner per pixel per pass -> plain RMW
__device__ __forceinline__ void add_sample(ctl_pixel* fb, const PathParams& P, f2 pX, spec col) {
    col.x = tmax(0.0f, col.x); col.y = tmax(0.0f, col.y); col.z = tmax(0.0f, col.z);
    int x = (int)floorf(pX.x), y = (int)floorf(pX.y);
    bool valid = !(isnan(col.x) || isnan(col.y) || isnan(col.z)) && isfinite(col.x) && isfinite(col.y) &&
                 isfinite(col.z) && col.x >= 0.0f && col.y >= 0.0f && col.z >= 0.0f;
    if (x >= 0 && x < (int)P.width && y >= 0 && y < (int)P.height && valid) {
        ctl_pixel* pp = fb + (size_t)y * P.width + x;
        pp->rgb[0] += col.x;
        pp->rgb[1] += col.y;
        pp->rgb[2] += col.z;
        pp->weight_sum += 1.0f;
    }
}

// Work item k of a pass covers pixel work_pixel(k).  Its finished sample lands
// on floor(pX) (Image::AddSample, Engine/Image.cu:22-44), which is the pixel
// itself or, when the jitter rounds up, its right / lower / lower-right
// neighbour, so two samples of one pass can meet on a pixel.  The path kernels
// therefore never add into the framebuffer: each work item stores its sample
// in its own slot (rgb, code), and fold_samples_kernel adds, per target pixel,
// the samples that landed there in work-item order, pass by pass -- the
// additions and their order of one sequential AddSample per work item.
// code: 0 = no sample (dropped as AddSample drops it), 1 + dx + 2 dy = landed
// on (px + dx, py + dy).
// A kernel's by-value record argument read in place from the kernel-argument
// segment (device pass; `arg` itself on the host pass, which never runs it).
// off = the argument's byte offset among the explicit arguments, laid out in
// order at their natural alignment (kernarg_next).
template <class T>
__device__ __forceinline__ const T& kernarg_ref(const T& arg, size_t off) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)arg;
    return *reinterpret_cast<const T*>((const char*)__builtin_amdgcn_kernarg_segment_ptr() + off);
#else
    (void)off;
    return arg;
#endif
}
// offset of the argument of type B that follows an argument of type A at offset off
template <class A, class B>
constexpr size_t kernarg_next(size_t off) {
    return (off + sizeof(A) + alignof(B) - 1) / alignof(B) * alignof(B);
}

struct SampleSlots {
    float4* s;            // [pass slot][work item]
    uint32_t per_pass;    // work items of one pass
    uint32_t inv;         // min(floor(2^32 / per_pass), 2^32 - 1): k / per_pass in one mul_hi (split)
    // k -> (pass slot, work item of the pass): the mul_hi quotient is exact or
    // one short (k < 2^32), fixed by one compare
    __device__ __forceinline__ void split(uint32_t k, uint32_t& ps, uint32_t& kk) const {
        ps = __umulhi(k, inv);
        kk = k - ps * per_pass;
        if (kk >= per_pass) { kk -= per_pass; ps++; }
    }
};
inline SampleSlots make_slots(float4* s, uint32_t per_pass) {
    const uint64_t q = per_pass ? (1ull << 32) / per_pass : 0;
    return SampleSlots{s, per_pass, (uint32_t)(q > 0xffffffffull ? 0xffffffffull : q)};
}
__device__ __forceinline__ void store_sample(const PathParams& P, const SampleSlots& S, uint32_t ps, uint32_t kk,
                                             uint32_t px, uint32_t py, f2 pX, spec col) {
    col.x = tmax(0.0f, col.x); col.y = tmax(0.0f, col.y); col.z = tmax(0.0f, col.z);
    const int x = (int)floorf(pX.x), y = (int)floorf(pX.y);
    const bool valid = !(isnan(col.x) || isnan(col.y) || isnan(col.z)) && isfinite(col.x) && isfinite(col.y) &&
                       isfinite(col.z) && col.x >= 0.0f && col.y >= 0.0f && col.z >= 0.0f;
    const int dx = x - (int)px, dy = y - (int)py;
    float code = 0.0f;
    if (x >= 0 && x < (int)P.width && y >= 0 && y < (int)P.height && valid && (dx | dy) >= 0 && dx <= 1 && dy <= 1)
        code = (float)(1 + dx + 2 * dy);
    S.s[(size_t)ps * S.per_pass + kk] = make_float4(col.x, col.y, col.z, code);
}

// store_sample in two halves, for a kernel that knows the pixel only when the path
// starts (the block-list pass, whose item -> pixel map goes through tables): the
// landing code from the pixel and its jittered position, and the store from the
// code once the radiance is known.  Together they write what store_sample writes.
__device__ __forceinline__ uint32_t landing_code(const PathParams& P, uint32_t px, uint32_t py, f2 pX) {
    const int x = (int)floorf(pX.x), y = (int)floorf(pX.y);
    const int dx = x - (int)px, dy = y - (int)py;
    const bool in = x >= 0 && x < (int)P.width && y >= 0 && y < (int)P.height && (dx | dy) >= 0 && dx <= 1 && dy <= 1;
    return in ? (uint32_t)(1 + dx + 2 * dy) : 0u;
}
__device__ __forceinline__ void store_sample_coded(const SampleSlots& S, uint32_t k, uint32_t code, spec col) {
    col.x = tmax(0.0f, col.x); col.y = tmax(0.0f, col.y); col.z = tmax(0.0f, col.z);
    const bool valid = !(isnan(col.x) || isnan(col.y) || isnan(col.z)) && isfinite(col.x) && isfinite(col.y) &&
                       isfinite(col.z) && col.x >= 0.0f && col.y >= 0.0f && col.z >= 0.0f;
    S.s[k] = make_float4(col.x, col.y, col.z, valid ? (float)code : 0.0f);
}

// Apron item g keeps its path only when the sample lands inside its tile.
__device__ __forceinline__ bool apron_keep(const PathParams& P, uint64_t g, f2 pX) {
    if (!P.apron || g < P.owned_items) return true;
    uint32_t px, py, x0, y0;
    apron_pixel(P, g - P.owned_items, px, py, x0, y0);
    const float lx = floorf(pX.x), ly = floorf(pX.y);
    return lx >= (float)x0 && lx < (float)(x0 + P.tile_size) && ly >= (float)y0 && ly < (float)(y0 + P.tile_size);
}

// Work item of source pixel (sx, sy) for a target pixel of tile (x0, y0) owned
// by this rank: its own item, or the tile's apron item when another rank owns it.
__device__ __forceinline__ bool source_item(const PathParams& P, uint32_t sx, uint32_t sy, uint32_t x0, uint32_t y0,
                                            uint32_t& k);

// inverse of work_pixel: owned pixel -> work item (false when another rank owns it)
__device__ __forceinline__ bool pixel_work(const PathParams& P, uint32_t x, uint32_t y, uint32_t& k) {
    const uint32_t ts = P.tile_size;
    const uint32_t tile = (y / ts) * P.tiles_x + x / ts;
    if (tile % P.num_ranks != P.rank) return false;
    const uint32_t xx = x % ts, yy = y % ts;
    k = (tile / P.num_ranks) * ts * ts + ((yy / 8) * (ts / 8) + xx / 8) * 64 + (yy % 8) * 8 + xx % 8;
    return true;
}

__device__ __forceinline__ bool source_item(const PathParams& P, uint32_t sx, uint32_t sy, uint32_t x0, uint32_t y0,
                                            uint32_t& k) {
    if (pixel_work(P, sx, sy, k)) return true;
    if (!P.apron) return false;
    const uint32_t ts = P.tile_size;
    const uint32_t tile = (y0 / ts) * P.tiles_x + x0 / ts;
    uint32_t i;
    if (sx + 1 == x0 && sy + 1 == y0) i = 2 * ts;
    else if (sx + 1 == x0) i = sy - y0;
    else i = ts + (sx - x0);
    k = P.owned_items + (tile / P.num_ranks) * P.apron + i;
    return true;
}

// Ownership policies of the persistent path kernel and the fold: which tiles a
// pass renders and where a pixel's work item lives.
//   OwnModulo  tile % num_ranks == rank, slot tile / num_ranks (the functions
//              above; `T` unused), every pass but a block-list one;
//   OwnList    the blocks of a list (ctl_render_pass_blocks), through device
//              tables at T (own_list_words words): slot -> the block's pixel
//              origin (x0, y0), block -> slot (kUnlisted when absent), slot ->
//              multiplicity.
// A list pass numbers its work items like an N-rank pass: owned_items pixels of
// the listed blocks by slot, then apron items per slot (P.apron = 2 ts + 1)
// for the samples that stray in from unlisted neighbours; an apron item whose
// pixel lies in a listed block is skipped (that block's own item covers it).
// The table lookups are per tile, so an 8x8 pixel group reads one entry; a
// wave's refilled lanes hold non-consecutive items, so they are per-lane loads.
// The origin table spares the refill the two divisions by tiles_x.
constexpr uint32_t kUnlisted = 0xffffffffu;
struct OwnModulo {
    static __device__ __forceinline__ bool work_pixel(const PathParams& P, const uint32_t*, uint64_t g, uint32_t& px,
                                                      uint32_t& py) {
        return ctl::work_pixel(P, g, px, py);
    }
    static __device__ __forceinline__ bool apron_keep(const PathParams& P, const uint32_t*, uint64_t g, f2 pX) {
        return ctl::apron_keep(P, g, pX);
    }
};
struct OwnList {
    // table layout in words, nt = num_tiles: [0, 2 nt) origins, [2 nt, 3 nt) block -> slot, [3 nt, 4 nt) multiplicity
    static __host__ __device__ constexpr size_t words(uint32_t nt) { return 4 * (size_t)nt; }
    static __host__ __device__ constexpr size_t slot_of_off(uint32_t nt) { return 2 * (size_t)nt; }
    static __host__ __device__ constexpr size_t mult_off(uint32_t nt) { return 3 * (size_t)nt; }
    // slot j < listed blocks <= num_tiles (the host bounds the work items)
    static __device__ __forceinline__ uint2 origin(const uint32_t* T, uint32_t j) {
        return reinterpret_cast<const uint2*>(T)[j];
    }
    static __device__ __forceinline__ uint32_t slot_of(const PathParams& P, const uint32_t* T, uint32_t x, uint32_t y) {
        return T[slot_of_off(P.num_tiles) + (y / P.tile_size) * P.tiles_x + x / P.tile_size];   // x < width, y < height
    }
    // Branch-free, both table reads unconditional (indices clamped into the tables):
    // the refill stays one straight-line block, as the modulo form's is -- with the
    // reads under branches the FULL kernels spill 9 more VGPRs
    // (profiles/adaptive_kernel_resources.txt).
    static __device__ __forceinline__ bool work_pixel(const PathParams& P, const uint32_t* T, uint32_t g, uint32_t& px,
                                                      uint32_t& py) {
        const uint32_t ts = P.tile_size;
        const bool ap = g >= P.owned_items;
        const uint32_t a = g - P.owned_items;                       // apron item (when ap)
        const uint32_t j = ap ? a / P.apron : g / (ts * ts);        // slot < listed blocks either way
        const uint2 o = origin(T, j);
        // the slot's own pixel
        const uint32_t w = g % (ts * ts), groupsPerRow = ts / 8, grp = w / 64, lane = w % 64;
        const uint32_t ox = o.x + (grp % groupsPerRow) * 8 + lane % 8, oy = o.y + (grp / groupsPerRow) * 8 + lane / 8;
        // the slot's apron pixel: left column, top row, corner (wraps below 0 are caught by the bounds)
        const uint32_t i = a % P.apron;
        const uint32_t ax = i < ts ? o.x - 1 : i < 2 * ts ? o.x + (i - ts) : o.x - 1;
        const uint32_t ay = i < ts ? o.y + i : o.y - 1;
        const bool ain = ax < P.width && ay < P.height;            // o.x - 1 with o.x == 0 is 2^32 - 1: outside
        const uint32_t t2 = ap && ain ? (ay / ts) * P.tiles_x + ax / ts : 0u;
        const uint32_t s2 = T[slot_of_off(P.num_tiles) + t2];
        px = ap ? ax : ox;
        py = ap ? ay : oy;
        // a listed block's pixel has its own item
        return ap ? ain && s2 == kUnlisted : ox < P.width && oy < P.height;
    }
    static __device__ __forceinline__ bool apron_keep(const PathParams& P, const uint32_t* T, uint32_t g, f2 pX) {
        if (g < P.owned_items) return true;
        const uint2 o = origin(T, (g - P.owned_items) / P.apron);
        const float lx = floorf(pX.x), ly = floorf(pX.y);
        return lx >= (float)o.x && lx < (float)(o.x + P.tile_size) && ly >= (float)o.y && ly < (float)(o.y + P.tile_size);
    }
    // Work item of source pixel (sx, sy) for a target pixel of the listed block in
    // slot `tslot` at (x0, y0): its own item when its block is listed, else the
    // target block's apron item.
    static __device__ __forceinline__ uint32_t source_item(const PathParams& P, const uint32_t* T, uint32_t sx,
                                                           uint32_t sy, uint32_t tslot, uint32_t x0, uint32_t y0) {
        const uint32_t ts = P.tile_size;
        const uint32_t slot = slot_of(P, T, sx, sy);
        if (slot != kUnlisted) {
            const uint32_t xx = sx % ts, yy = sy % ts;
            return slot * ts * ts + ((yy / 8) * (ts / 8) + xx / 8) * 64 + (yy % 8) * 8 + xx % 8;
        }
        uint32_t i;
        if (sx + 1 == x0 && sy + 1 == y0) i = 2 * ts;
        else if (sx + 1 == x0) i = sy - y0;
        else i = ts + (sx - x0);
        return P.owned_items + tslot * P.apron + i;
    }
};

}  // namespace ctl

#include "shading.h"   // the shading levels, the integrators' shared steps, shade_hit

namespace ctl {

// Wavefront path state, structure of arrays (capacity = paths per pass).
struct WfState {
    float4* o;        // ray origin xyz | w: brdf_pdf
    float4* d;        // ray direction xyz | w: unused
    float4* cl;       // accumulated radiance xyz | w: pX.x
    float4* cf;       // throughput xyz | w: pX.y
    float4* wo;       // persistent BSDF wo xyz | w: last_nor.x
    float2* ln;       // last_nor.yz
    uint4* meta;      // x: pixel idx, y: d1 | d2 << 16, z: depth | specular << 16, w: has_partials
    float4* part;     // dudx, dudy, dvdx, dvdy (first-hit partials, kept for the path)
    float4* hit;      // t, u, v, tri bits
    uint32_t* hit_node;
    uint32_t* q[2];   // extension-ray queues (path indices), ping-pong
    uint32_t* sq;     // shadow queue (path indices)
    float4* sh_o;     // shadow ray origin | w: tmax (any-hit: dist - eps)
    float4* sh_d;     // shadow ray direction | w: dist
    float4* sh_val;   // contribution to add if unoccluded | w: terminated flag
    uint32_t* sh_occ; // occlusion result
    uint32_t* counts; // [2 * bounce + {0: ext queue, 1: shadow queue}]
    size_t capacity;
};

struct WptBuffers;
struct AnimState;
struct ImageState;
struct LbvhScratch;

// The two regions ctl_scene_rebuild_mesh appended to the node, Woop, index and
// 4-wide arrays for one mesh (anim.hip): each rebuild builds into the one the
// mesh is not using.  Element offsets into the device arrays.
struct MeshRegion {
    bool has = false;
    int cur = -1;                               // the region the mesh's record points to (-1: the uploaded range)
    uint64_t node0[2] = {0, 0}, entry0[2] = {0, 0}, wide0[2] = {0, 0};
};

// Device arrays of an uploaded scene (scene_dev.hip): one allocation per
// KernelDynamicScene stream, reused by ctl_scene_update while it fits.
// SA_LIGHTS is allocated whole at its first upload and never grows: CTL_MAX_NUM_LIGHTS ctl_light slots,
// then the scene's ctl_volume at byte kVolumeAt (traverse.h scene_volume reads it there, ctl_ctx::d_volume
// points at it), then the scene's ctl_sensor at byte kSensorAt (traverse.h scene_sensor).  Its `bytes` counts
// the uploaded lights only.  Whoever re-puts or resizes SA_LIGHTS keeps the tail: scene_dev.hip commit_arrays
// writes the volume record back after every lights upload, and the sensor record on every commit.
constexpr size_t kVolumeAt = CTL_MAX_NUM_LIGHTS * sizeof(ctl_light);
constexpr size_t kSensorAt = kVolumeAt + sizeof(ctl_volume);
constexpr size_t kLightsArrayBytes = kSensorAt + sizeof(ctl_sensor);
static_assert(kVolumeAt % 16 == 0, "the volume record is read at a 16-byte aligned address behind the light slots");
static_assert(kSensorAt % 16 == 0, "the sensor record is read at a 16-byte aligned address behind the volume record");
enum SceneArr : int {
    SA_BVH, SA_WOOP, SA_IDX, SA_TRI, SA_MATS, SA_MESHES, SA_NODES, SA_SBVH, SA_XF, SA_IXF, SA_LIGHTS, SA_LTRIS,
    SA_LCDF, SA_LUT, SA_TEX, SA_TEXDATA, SA_ENV, SA_ENVDATA, SA_WBVH, SA_SWBVH, SA_WBASE, SA_MATX,
    SA_COUNT
};
struct SceneArray {
    DevArray<char> mem;   // cap(): bytes allocated
    size_t bytes = 0;     // bytes of the current contents
};

}  // namespace ctl

struct ctl_ctx {
    int device = 0;
    std::string err;
    ctl::SceneArray sarr[ctl::SA_COUNT];
    std::vector<uint32_t> h_wbase;              // host copy of the mesh wide-tree bases
    int stack_mesh_bin = 0, stack_mesh_wide = 0;// worst-case mesh-level stacks (bvh_wide.h)
    int stack_top_bin = -1, stack_top_wide = -1;// top level (-1: no instance tree)
    uint32_t tree_flags = 0;                    // CTL_SCENE_BINARY_BVH / WIDE_QUANT the trees were built for
    uint32_t n_anim_meshes = 0;
    bool device_eps = false;                    // ray_eps derived on the device (set_transform / animate)
    bool device_edited = false;                 // set_transform / animate rewrote device arrays since the upload
    ctl::DevScene scene{};
    bool has_scene = false;
    bool half_quirk = false;
    bool has_delta = false;                     // some uploaded material has a delta lobe (prim.hip)
    uint32_t material_level = 0;                // shading level the materials and the environment ask for
    bool has_delta_light = false;               // some uploaded light is a point, spot or distant light
    ctl_volume h_volume{};                      // host copy of that record (all zero without one)
    const ctl_volume* d_volume = nullptr;       // the uploaded scene's medium (behind the light slots of SA_LIGHTS), null without one
    ctl_sensor h_sensor = ctl::sensor_default(); // host copy of the uploaded sensor record (the perspective one without a record)
    uint32_t nseq = 4096, len = 30;
    ctl::DevPool fixed;                         // owns the arrays allocated once by ctl_create
    float* d_s1[2] = {nullptr, nullptr};        // (fixed)
    float2* d_s2[2] = {nullptr, nullptr};       // (fixed)
    // ctl_render_passes: sampler tables of every pass of one launch, and the
    // per-pass sample slices of the owned tiles (folded into the caller's
    // framebuffer in pass order)
    ctl::DevArray<float> d_mt1;
    ctl::DevArray<float2> d_mt2;
    ctl::DevArray<float4> d_slices;             // SampleSlots of the path kernels (common.h)
    ctl::PinnedArray<float> h_s1[2], h_s2[2];
    ctl::Event ev[2];
    int next_buf = 0, active = -1;
    unsigned long long* d_counters = nullptr;   // [0] rays [1] overflow [2..4] stats [7], [15] tail hand-over (fixed)
    ctl::PinnedArray<unsigned long long> h_overflow;   // host copy of d_counters[1], read at ctl_sync
    bool overflow_seen = false;                 // sticky: a traversal stack overflowed since the last reset
    // 64-bit work cursors ([0] batch intersect [1] path pass [2] prim pass): resident
    // lanes fetch once more after the work runs out, which a 32-bit cursor
    // near 2^32 items would wrap
    unsigned long long* d_cursors = nullptr;    // (fixed)
    std::vector<std::pair<const void*, std::pair<size_t, int>>> resident;   // resident_blocks cache
    ctl::Event pass_ev[2];                      // bracket the last render pass (ctl_last_pass_ms)
    bool pass_timed = false;
    size_t wide_nodes = 0;
    int stack_bound = 0;                        // worst-case traversal stack of the uploaded scene
    ctl::DevArray<uint8_t> d_tile_flags;        // PixelVarianceBuffer block flags
    // ctl_render_pass_blocks: the OwnList tables (OwnList::words), filled in one half
    // of the pinned staging buffer and uploaded stream-ordered.  The halves alternate
    // and block_ev[h] marks half h's last upload, so the host waits only for the
    // upload of two calls ago and a caller can queue list passes without stalling.
    ctl::DevArray<uint32_t> d_block_tbl;        // OwnList::words(tiles allocated for)
    ctl::PinnedArray<uint32_t> h_block_tbl;     // two halves of d_block_tbl.cap() words
    ctl::Event block_ev[2];
    bool block_ev_set[2] = {false, false};      // block_ev[h] has been recorded
    uint32_t block_half = 0;                    // the half the next call fills
    uint32_t* d_powers = nullptr;               // XORWOW step powers for sampler_kernel (fixed)
    ctl::WfState wf{};
    ctl::DevPool wf_pool;                       // owns wf's arrays
    ctl::WptBuffers* wpt = nullptr;             // WavefrontPathTracer queues (wpt.hip)
    ctl::AnimState* anim = nullptr;             // animated meshes, refit plans (anim.hip)
    ctl::ImageState* img = nullptr;             // image pipeline scratch and NLM weights (pipeline.hip)
    // ctl_scene_rebuild_mesh: the builder's scratch (lbvh.hip), the regions appended past
    // the uploaded arrays (elements; the uploaded lengths stay in sarr[].bytes), a host copy
    // of the uploaded mesh records and the per-mesh stack bounds behind stack_mesh_*
    ctl::LbvhScratch* lbvh = nullptr;
    std::vector<ctl::MeshRegion> regions;
    uint64_t extra_nodes = 0, extra_entries = 0, extra_wide = 0;
    std::vector<ctl_kernel_mesh> h_meshes;
    std::vector<int> mesh_bin_bound, mesh_wide_bound;
    float rebuild_ms[2] = {0.0f, 0.0f};         // host time of the last rebuild's two phases (ctl_last_rebuild_ms)
    uint64_t n_tri_data = 0, n_woop = 0, n_bvh_nodes = 0, n_scene_bvh = 0;   // uploaded array lengths
    int cu_count = 256;
    // Speculative DoPass windows (ctl_render_pass): the reference's host loop
    // renders one pass per call (Tracer.h:209-248); once the calls follow each
    // other with consecutive sampler passes and nothing else changing, one call
    // renders the next passes too in one launch (their samples wait in the sample
    // slots) and the following calls only fold them.  Anything that changes the
    // scene, the tables, the parameters, the framebuffer or the stream, or uses
    // the slots, drops the pending passes.
    uint64_t scene_epoch = 0;                   // bumped by every scene / table change
    int64_t tables_pass = -1;                   // pass of the active sampler tables (-1: uploaded tables)
    struct Spec {
        bool pending = false;                   // slots hold passes [next, end) of the window
        int64_t first = 0, next = 0, end = 0;
        bool last_valid = false;                // the previous ctl_render_pass call, for the pattern
        int64_t last_pass = 0;
        ctl_pt_params params{};
        const void* fb = nullptr;
        const void* stream = nullptr;
        uint64_t epoch = 0;
        uint32_t streak = 0;                    // windows consumed in a row: their length doubles up to 8
        uint64_t per_pass = 0;
    } spec;
};

namespace ctl {
// Persistent grids = exactly the co-resident blocks (occupancy from the
// compiled register/LDS footprint x CU count): no block waits for a slot and
// the atomic work cursor spreads the pass evenly over all CUs.  Cached per
// context (a context is bound to one device and one host thread at a time).
template <class K>
int resident_blocks(ctl_ctx* c, K kernel, size_t lds) {
    const void* key = reinterpret_cast<const void*>(kernel);
    for (const auto& e : c->resident) if (e.first == key && e.second.first == lds) return e.second.second;
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kBlock, lds) != hipSuccess || per_cu <= 0)
        per_cu = 2;
    const int nb = per_cu * c->cu_count;
    c->resident.push_back({key, {lds, nb}});
    return nb;
}
// The grid of a persistent launch: the resident blocks, at most bpc blocks per
// CU when bpc > 0, and no more than the `want` blocks the work fills.
template <class K>
dim3 resident_grid(ctl_ctx* c, K kernel, size_t lds, uint64_t want, int bpc = 0) {
    int nb = resident_blocks(c, kernel, lds);
    if (bpc > 0) nb = std::min(nb, bpc * c->cu_count);
    return dim3((unsigned)std::min<uint64_t>(nb, want));
}

// A failed HIP call of a C-ABI function: the call's text (`what`) and HIP's
// message into the context's error string, CTL_ERR_HIP to the caller.
#define CTL_HIP_AS(ctx, call, what)                                                        \
    do {                                                                                   \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess) {                                                            \
            (ctx)->err = std::string(what) + ": " + hipGetErrorString(e_);                 \
            return CTL_ERR_HIP;                                                            \
        }                                                                                  \
    } while (0)
#define CTL_HIP(ctx, call) CTL_HIP_AS(ctx, call, #call)

// scene_dev.hip: drops the device scene
void free_scene(ctl_ctx* c);
// wavefront.hip
int wavefront_pass(ctl_ctx* c, const PathParams& P, const SampleSlots& SS, bool stats, hipStream_t s);
// anim.hip
struct WideNode;
int anim_setup(ctl_ctx* c, const ctl_scene_desc* d, const std::vector<WideNode>& wn, const std::vector<uint32_t>& wbase,
               const std::vector<WideNode>& sw);
void anim_free(ctl_ctx* c);
// lbvh.hip: the device mesh builder behind ctl_scene_rebuild_mesh
constexpr uint32_t kLbvhResWords = 16;   // [6] non-finite flag [7] wide stack bound [8] root height [9..14] mesh box
int lbvh_reserve(ctl_ctx* c, uint32_t n);
int lbvh_build(ctl_ctx* c, const float* d_pos, uint32_t n, void* nodes, void* woop, uint32_t* idx, void* wide,
               hipStream_t s);
const uint32_t* lbvh_result(const ctl_ctx* c);
const uint32_t* lbvh_result_dev(const ctl_ctx* c);
void lbvh_free(ctl_ctx* c);
// wpt.hip
int wpt_pass(ctl_ctx* c, const ctl_wpt_params* p, ctl_pixel* fb, hipStream_t s);
void wpt_free(ctl_ctx* c);
// pipeline.hip
void image_free(ctl_ctx* c);
// ctl_trace.hip: the batch traversal launch and the ray counter, for wpt.hip
// (rays, hits)[0, n) and, in the same launch, (rays2, hits2)[0, n2)
int intersect_launch(ctl_ctx* c, int64_t n, const ctl_ray* rays, ctl_hit* hits, int32_t any_hit, hipStream_t s,
                     int64_t n2 = 0, const ctl_ray* rays2 = nullptr, ctl_hit* hits2 = nullptr,
                     const uint32_t* dcount = nullptr, uint32_t band_w = 0);
int count_rays(ctl_ctx* c, uint64_t n, hipStream_t s);
// path_media.hip: launch_path / launch_path_blocks (path_kernels.h) of the level kShadeMedia;
// false, and nothing launched, when the uploaded scene has another level
bool media_launch_path(ctl_ctx* c, bool persistent, bool stats, const PathParams& P, const float* s1, const float2* s2,
                       uint64_t threads, uint64_t want, dim3 grid, unsigned long long* cursor, ctl_pixel* fb, SampleSlots PS,
                       uint32_t tbl, hipStream_t s);
bool media_launch_blocks(ctl_ctx* c, const PathParams& P, const float* s1, const float2* s2, uint64_t items, uint64_t want,
                         unsigned long long* cursor, SampleSlots PS, const uint32_t* own_tbl, hipStream_t s);
// path_sensors.hip: the same for the level kShadeSensors, and the camera-ray batch of ctl_camera_rays at that level
bool sensors_launch_path(ctl_ctx* c, bool persistent, bool stats, const PathParams& P, const float* s1, const float2* s2,
                         uint64_t threads, uint64_t want, dim3 grid, unsigned long long* cursor, ctl_pixel* fb,
                         SampleSlots PS, uint32_t tbl, hipStream_t s);
bool sensors_launch_blocks(ctl_ctx* c, const PathParams& P, const float* s1, const float2* s2, uint64_t items,
                           uint64_t want, unsigned long long* cursor, SampleSlots PS, const uint32_t* own_tbl,
                           hipStream_t s);
bool sensors_launch_camera_rays(ctl_ctx* c, const PathParams& P, const float* s1, const float2* s2, uint64_t items,
                                ctl_ray* rays, hipStream_t s);
}
