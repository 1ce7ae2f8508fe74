// lbvh.hip — a mesh's trees built on the device from triangle positions
// (ctl_scene_rebuild_mesh): what Mesh::CompileMesh + ConstructBVH do on the host
// (Engine/Mesh.cpp, Engine/SpatialStructures/BVH), for geometry already resident.
//
// An LBVH in the form of Karras, "Maximizing Parallelism in the Construction of
// BVHs, Octrees, and k-d Trees" (HPG 2012).  Every step is a function of the
// positions alone, so two builds of one input give the same bytes and a CPU
// restatement (tests/lbvh_ref.py) predicts every byte:
//
//   box     per triangle: the box by fp32 min / max of the three vertices, each
//           bound + 0.0f (no -0.0 in any box, so min / max are order-free), the
//           centroid proxy lo + hi; the proxies' box by atomic min / max on
//           order-preserving integer codes; a flag for non-finite input (a
//           coordinate, or a proxy that overflows)
//   key     per axis q = (c - cb_lo) / (cb_hi - cb_lo) (0 on an axis of zero
//           extent), code = min(2^21 - 1, (uint32_t)(q * 2097152.0f)), 63-bit
//           Morton key: x in bits 3k + 2, y in 3k + 1, z in 3k
//   sort    stable ascending radix sort of (key, triangle) over all 64 bits
//           (rocPRIM; begin_bit = 0, see probes/rocprim_sort_check.hip): equal
//           keys stay in triangle order
//   tree    one thread per inner node i in [0, n - 2]: delta(i, j) =
//           clz64(key_i ^ key_j), 64 + clz32(i ^ j) on equal keys, -1 out of
//           range; Karras's direction, range and split; child 0 the left range;
//           inner child word 4 x node, leaf child word ~entry (the sorted
//           position); parent words (4 x parent, the root 0xFFFFFFFF)
//   leaves  one thread per entry: Woop record (woop_set_hd), index word
//           (triangle << 1 | 1: leaves of one triangle), leaf box
//   fit     bottom-up, one arrival counter per inner node: the second child to
//           arrive writes the node's two child boxes (BVHNodeData's
//           interleaving) and the node's record (box = min / max of the two,
//           surface area 2 (dx dy + dy dz + dz dx) summed in that order,
//           height), then climbs.  Records go through SC1 buffer accesses and
//           the arrival is a relaxed agent-scope atomic behind s_waitcnt
//           vmcnt(0), as in anim.hip's climb.  The root's record is the mesh
//           box and the binary stack bound (1 + height).
//   4-wide  greedy collapse, level by level from binary node 0: a wide node
//           starts from a binary node's two children and opens the inner child
//           of largest surface area (a tie: the lowest slot) until it has four
//           children or no inner child; the opened child's slot takes its child
//           0, its child 1 the first free slot.  A level's launch strides over
//           the list of binary nodes the level before left (appended with one
//           atomic add per wave: the list's order shows in no output), at most
//           91 launches (the keys and indices give at most 91 distinct values
//           of delta along a path).  Wide nodes are numbered by an
//           exclusive prefix sum, over the binary node index, of "this binary
//           node starts a wide node" (rocPRIM): no atomically allocated index;
//           binary node 0 starts wide node 0.  The wide stack bound
//           1 + sum(children - 1) rides along the levels (atomic max).
//           Leaf children carry the counted code ~((entry << 3) | 1), empty
//           slots quiet-NaN boxes and 0x76543210, the pad is zero.
//
// The SAH-optimal collapse stays on the host (host/bvh_wide.cpp); so do leaf
// merging, rotations and spatial splits.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cfloat>

#include "common.h"
#include "../ctl_anim.h"
#include "../host/bvh_wide.h"

namespace ctl {

struct LbvhScratch {
    uint32_t cap = 0;               // triangles the arrays are sized for (0: the pointers below are not valid)
    uint64_t* keys[2] = {nullptr, nullptr};
    uint32_t* vals[2] = {nullptr, nullptr};
    uint32_t* lpar = nullptr;       // per entry: its parent node
    float* lbox = nullptr;          // per entry: {lo xyz, hi.x} {hi.y, hi.z, 0, 0}
    float* nbox = nullptr;          // per inner node: {lo xyz, hi.x} {hi.y, hi.z, area, height}
    uint32_t* cnt = nullptr;        // arrival counters
    uint32_t* front = nullptr;      // the collapse's level lists (binary nodes), alternating with widx
    uint32_t* below = nullptr;      // per wide-node start: stack entries below it
    uint32_t* flag = nullptr;       // per inner node: starts a wide node
    uint32_t* widx = nullptr;       // exclusive prefix sum of flag
    int4* wkids = nullptr;          // per wide-node start: its slots' binary child words
    char* tmp = nullptr;            // rocPRIM temporary storage
    size_t tmp_bytes = 0;
    DevPool pool;                   // owns the arrays above
    DevArray<uint32_t> d_res;       // kLbvhResWords words (LbvhRes), then the level counts; kept across a regrow
    PinnedArray<uint32_t> h_res;    // copy of the result words
};

namespace {

constexpr int kLB = 256;
constexpr int32_t kSent = 0x76543210;
constexpr uint32_t kMaxLevels = 91;
constexpr uint32_t kLevelWords = 96;   // per-level counts behind the result words (levels 0 .. kMaxLevels)
// result words: [0..2] proxy box min codes, [3..5] max codes, [6] non-finite flag,
// [7] wide stack bound, [8] root height, [9..14] mesh box
enum : int { kResFlag = 6, kResWide = 7, kResHeight = 8, kResBox = 9 };

// order-preserving code of a float (no NaN, no -0.0 among the coded values)
__device__ __forceinline__ uint32_t fcode(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : b | 0x80000000u;
}
__device__ __forceinline__ float fdecode(uint32_t c) {
    return __uint_as_float((c & 0x80000000u) ? c & 0x7fffffffu : ~c);
}

struct TriBox {
    float lo[3], hi[3];
};
// v0 v1 v2 of triangle t; the bounds + 0.0f turn a -0.0 into +0.0
__device__ __forceinline__ TriBox tri_box(const float* __restrict__ pos, uint32_t t, f3& a, f3& b, f3& c) {
    const float* p = pos + 9 * (size_t)t;
    a = mk3(p[0], p[1], p[2]);
    b = mk3(p[3], p[4], p[5]);
    c = mk3(p[6], p[7], p[8]);
    TriBox r;
    r.lo[0] = tmin(tmin(a.x, b.x), c.x) + 0.0f; r.hi[0] = tmax(tmax(a.x, b.x), c.x) + 0.0f;
    r.lo[1] = tmin(tmin(a.y, b.y), c.y) + 0.0f; r.hi[1] = tmax(tmax(a.y, b.y), c.y) + 0.0f;
    r.lo[2] = tmin(tmin(a.z, b.z), c.z) + 0.0f; r.hi[2] = tmax(tmax(a.z, b.z), c.z) + 0.0f;
    return r;
}

__device__ __forceinline__ bool tri_finite(f3 a, f3 b, f3 c) {
    return isfinite(a.x) && isfinite(a.y) && isfinite(a.z) && isfinite(b.x) && isfinite(b.y) && isfinite(b.z) &&
           isfinite(c.x) && isfinite(c.y) && isfinite(c.z);
}

__global__ void lbvh_init_kernel(uint32_t* res, uint32_t* front, uint32_t* below) {
    for (int k = 0; k < 3; k++) { res[k] = 0xffffffffu; res[3 + k] = 0u; }
    for (int k = kResFlag; k < kResBox + 6; k++) res[k] = 0u;
    uint32_t* fcount = res + kLbvhResWords;   // nodes per level of the collapse
    for (uint32_t k = 0; k < kLevelWords; k++) fcount[k] = 0u;
    fcount[0] = 1u;
    front[0] = 0u;                            // level 0: binary node 0
    below[0] = 1u;
}

// box: the centroid proxies' box and the non-finite flag.  A fixed grid strides
// over the triangles and each block reduces in registers and LDS first: one
// atomic per word per block (one per wave cost 2.2 ms at 2 M triangles, all on
// one cache line).  min / max are order-free, so the grid does not show.
constexpr uint32_t kBoxBlocks = 1024;
__global__ __launch_bounds__(kLB) void lbvh_box_kernel(const float* __restrict__ pos, uint32_t n, uint32_t* res) {
    uint32_t mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
    bool bad = false;
    for (uint32_t t = blockIdx.x * kLB + threadIdx.x; t < n; t += gridDim.x * kLB) {
        f3 a, b, c;
        const TriBox tb = tri_box(pos, t, a, b, c);
        bool tbad = !tri_finite(a, b, c);   // a NaN vertex can hide behind min / max
        float p[3];
        for (int k = 0; k < 3; k++) {
            p[k] = tb.lo[k] + tb.hi[k];
            tbad = tbad || !isfinite(p[k]);
        }
        bad = bad || tbad;
        if (!tbad)
            for (int k = 0; k < 3; k++) {
                const uint32_t code = fcode(p[k]);
                mn[k] = min(mn[k], code);
                mx[k] = max(mx[k], code);
            }
    }
    for (int off = 32; off > 0; off >>= 1)
        for (int k = 0; k < 3; k++) {
            mn[k] = min(mn[k], (uint32_t)__shfl_xor((int)mn[k], off));
            mx[k] = max(mx[k], (uint32_t)__shfl_xor((int)mx[k], off));
        }
    const bool any_bad = __ballot(bad) != 0;
    __shared__ uint32_t part[kLB / 64][7];
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        for (int k = 0; k < 3; k++) { part[wave][k] = mn[k]; part[wave][3 + k] = mx[k]; }
        part[wave][6] = any_bad ? 1u : 0u;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t flag = 0;
        for (int w = 0; w < kLB / 64; w++) {
            for (int k = 0; k < 3; k++) { mn[k] = min(mn[k], part[w][k]); mx[k] = max(mx[k], part[w][3 + k]); }
            flag |= part[w][6];
        }
        for (int k = 0; k < 3; k++) {
            if (mn[k] != 0xffffffffu) atomicMin(res + k, mn[k]);
            if (mx[k] != 0u) atomicMax(res + 3 + k, mx[k]);
        }
        if (flag) atomicOr(res + kResFlag, 1u);
    }
}

// a 21-bit code spread to every third bit
__device__ __forceinline__ uint64_t spread3(uint32_t v) {
    uint64_t x = v & 0x1fffffu;
    x = (x | x << 32) & 0x1f00000000ffffull;
    x = (x | x << 16) & 0x1f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

__global__ __launch_bounds__(kLB) void lbvh_key_kernel(const float* __restrict__ pos, uint32_t n,
                                                      const uint32_t* __restrict__ res, uint64_t* keys, uint32_t* vals) {
    const uint32_t t = blockIdx.x * kLB + threadIdx.x;
    if (t >= n) return;
    f3 a, b, c;
    const TriBox tb = tri_box(pos, t, a, b, c);
    uint32_t code[3];
    for (int k = 0; k < 3; k++) {
        const float lo = fdecode(res[k]), hi = fdecode(res[3 + k]);
        const float ext = hi - lo;
        const float q = ext == 0.0f ? 0.0f : ((tb.lo[k] + tb.hi[k]) - lo) / ext;
        code[k] = min(0x1fffffu, (uint32_t)(q * 2097152.0f));
    }
    keys[t] = spread3(code[0]) << 2 | spread3(code[1]) << 1 | spread3(code[2]);
    vals[t] = t;
}

__device__ __forceinline__ int lbvh_delta(const uint64_t* __restrict__ keys, uint64_t ki, int64_t i, int64_t j, int64_t n) {
    if (j < 0 || j >= n) return -1;
    const uint64_t x = ki ^ keys[j];
    return x ? __clzll((long long)x) : 64 + __clz((int)((uint32_t)i ^ (uint32_t)j));
}

// tree: node i's child words, its children's parent words
__global__ __launch_bounds__(kLB) void lbvh_tree_kernel(const uint64_t* __restrict__ keys, uint32_t n, float* nodes,
                                                       uint32_t* lpar) {
    const uint32_t ti = blockIdx.x * kLB + threadIdx.x;
    if (ti + 1 >= n) return;
    const int64_t i = ti, N = n;
    const uint64_t ki = keys[i];
    const int d = lbvh_delta(keys, ki, i, i + 1, N) > lbvh_delta(keys, ki, i, i - 1, N) ? 1 : -1;
    const int dmin = lbvh_delta(keys, ki, i, i - d, N);
    int64_t lmax = 2;
    while (lbvh_delta(keys, ki, i, i + lmax * d, N) > dmin) lmax *= 2;
    int64_t l = 0;
    for (int64_t t = lmax / 2; t >= 1; t /= 2)
        if (lbvh_delta(keys, ki, i, i + (l + t) * d, N) > dmin) l += t;
    const int64_t j = i + l * d;
    const int dnode = lbvh_delta(keys, ki, i, j, N);
    int64_t s = 0;
    for (int64_t t = (l + 1) >> 1;; t = (t + 1) >> 1) {
        if (lbvh_delta(keys, ki, i, i + (s + t) * d, N) > dnode) s += t;
        if (t <= 1) break;
    }
    const int64_t g = i + s * d + (d < 0 ? -1 : 0);
    const int64_t first = i < j ? i : j, last = i < j ? j : i;
    const bool leaf0 = first == g, leaf1 = last == g + 1;
    const int32_t c0 = leaf0 ? ~(int32_t)g : (int32_t)(4 * g), c1 = leaf1 ? ~(int32_t)(g + 1) : (int32_t)(4 * (g + 1));
    float* nd = nodes + 16 * (size_t)i;
    nd[12] = __int_as_float(c0);
    nd[13] = __int_as_float(c1);
    if (i == 0) nd[14] = __uint_as_float(0xffffffffu);
    nd[15] = 0.0f;
    if (leaf0) lpar[g] = (uint32_t)i; else nodes[16 * (size_t)g + 14] = __uint_as_float((uint32_t)(4 * i));
    if (leaf1) lpar[g + 1] = (uint32_t)i; else nodes[16 * (size_t)(g + 1) + 14] = __uint_as_float((uint32_t)(4 * i));
}

// leaves: entry e holds triangle vals[e]
__global__ __launch_bounds__(kLB) void lbvh_leaf_kernel(const float* __restrict__ pos, const uint32_t* __restrict__ vals,
                                                       uint32_t n, float4* woop, uint32_t* idx, float* lbox) {
    const uint32_t e = blockIdx.x * kLB + threadIdx.x;
    if (e >= n) return;
    const uint32_t t = min(vals[e], n - 1);   // a permutation of [0, n): the bound only guards the loads below
    f3 a, b, c;
    const TriBox tb = tri_box(pos, t, a, b, c);
    float w[12];
    woop_set_hd(a, b, c, w);
    woop[3 * (size_t)e] = make_float4(w[0], w[1], w[2], w[3]);
    woop[3 * (size_t)e + 1] = make_float4(w[4], w[5], w[6], w[7]);
    woop[3 * (size_t)e + 2] = make_float4(w[8], w[9], w[10], w[11]);
    idx[e] = t << 1 | 1u;
    float4* r = reinterpret_cast<float4*>(lbox + 8 * (size_t)e);
    r[0] = make_float4(tb.lo[0], tb.lo[1], tb.lo[2], tb.hi[0]);
    r[1] = make_float4(tb.hi[1], tb.hi[2], 0.0f, 0.0f);
}

// the records two threads of the fit launch share: SC1 buffer accesses
// (coherent across the XCDs' L2s access by access), as anim.hip's climb
constexpr int kSC1 = 16;
__device__ __forceinline__ float4 cld4(__amdgpu_buffer_rsrc_t r, uint32_t off) {
    return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, kSC1));
}
__device__ __forceinline__ void cst4(__amdgpu_buffer_rsrc_t r, uint32_t off, float4 v) {
    using v4u = __attribute__((ext_vector_type(4))) unsigned int;
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, v), r, off, 0, kSC1);
}

struct Rec {
    float lo[3], hi[3];
    uint32_t height;
};
__device__ __forceinline__ Rec rec_of(float4 a, float4 c) {
    return Rec{{a.x, a.y, a.z}, {a.w, c.x, c.y}, __float_as_uint(c.w)};
}

// fit: one thread per entry climbs; the second arrival at a node writes it
__global__ __launch_bounds__(kLB) void lbvh_fit_kernel(uint32_t n, float* nodes, const uint32_t* __restrict__ lpar,
                                                      const float* __restrict__ lbox, float* nbox, uint32_t* cnt,
                                                      uint32_t* res) {
    const uint32_t e = blockIdx.x * kLB + threadIdx.x;
    if (e >= n) return;
    const __amdgpu_buffer_rsrc_t R = __builtin_amdgcn_make_buffer_rsrc(nbox, 0, (int)(32u * (n - 1)), 0x00020000);
    uint32_t x = lpar[e];
    for (;;) {
        // the caller's coherent stores complete before it arrives; no load of the
        // first arrival's record is hoisted above the counter
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t old = __hip_atomic_fetch_add(cnt + x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("" ::: "memory");
        if (old == 0) return;
        float* nd = nodes + 16 * (size_t)x;
        const int32_t k[2] = {__float_as_int(nd[12]), __float_as_int(nd[13])};
        Rec r[2];
        for (int q = 0; q < 2; q++) {
            if (k[q] < 0) {
                const float4* l = reinterpret_cast<const float4*>(lbox + 8 * (size_t)(uint32_t)~k[q]);
                r[q] = rec_of(l[0], l[1]);
            } else {
                const uint32_t ch = (uint32_t)k[q] >> 2;
                r[q] = rec_of(cld4(R, 32u * ch), cld4(R, 32u * ch + 16u));
            }
        }
        float4* F = reinterpret_cast<float4*>(nd);
        F[0] = make_float4(r[0].lo[0], r[0].hi[0], r[0].lo[1], r[0].hi[1]);
        F[1] = make_float4(r[1].lo[0], r[1].hi[0], r[1].lo[1], r[1].hi[1]);
        F[2] = make_float4(r[0].lo[2], r[0].hi[2], r[1].lo[2], r[1].hi[2]);
        float lo[3], hi[3];
        for (int q = 0; q < 3; q++) { lo[q] = tmin(r[0].lo[q], r[1].lo[q]); hi[q] = tmax(r[0].hi[q], r[1].hi[q]); }
        const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
        const float area = 2.0f * (dx * dy + dy * dz + dz * dx);
        const uint32_t h = 1u + max(r[0].height, r[1].height);
        cst4(R, 32u * x, make_float4(lo[0], lo[1], lo[2], hi[0]));
        cst4(R, 32u * x + 16u, make_float4(hi[1], hi[2], area, __uint_as_float(h)));
        const int32_t p = __float_as_int(nd[14]);
        if (p < 0) {
            res[kResHeight] = h;
            for (int q = 0; q < 3; q++) { res[kResBox + q] = __float_as_uint(lo[q]); res[kResBox + 3 + q] = __float_as_uint(hi[q]); }
            return;
        }
        x = (uint32_t)p >> 2;
    }
}

// 4-wide, level L: each binary node of the level's list starts a wide node; its
// inner children that stay unopened go to the next level's list.  The lists are
// scratch: a node's place in them (one wave-aggregated atomic add per wave) shows
// in no output, the wide nodes are numbered by the prefix sum afterwards.  A
// fixed grid strides over the list, whose length is read on the device.
constexpr uint32_t kLevelBlocks = 1024;
__global__ __launch_bounds__(kLB) void lbvh_wide_level_kernel(uint32_t L, const float* __restrict__ nodes,
                                                             const float* __restrict__ nbox,
                                                             const uint32_t* __restrict__ src, uint32_t* dst,
                                                             uint32_t* below, uint32_t* flag, int4* wkids, uint32_t* res) {
    uint32_t* fcount = res + kLbvhResWords;
    const uint32_t count = fcount[L];
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t j0 = blockIdx.x * kLB + (threadIdx.x & ~63u); j0 < count; j0 += gridDim.x * kLB) {   // wave-uniform
        const bool act = j0 + lane < count;
        int32_t k[4] = {kSent, kSent, kSent, kSent};
        int nk = 0;
        uint32_t b = 0, here = 0;
        if (act) {
            b = src[j0 + lane];
            k[0] = __float_as_int(nodes[16 * (size_t)b + 12]);
            k[1] = __float_as_int(nodes[16 * (size_t)b + 13]);
            nk = 2;
            while (nk < 4) {
                int best = -1;
                float best_a = 0.0f;
                for (int q = 0; q < 4; q++) {
                    if (q >= nk || k[q] < 0) continue;
                    const float a = nbox[8 * (size_t)((uint32_t)k[q] >> 2) + 6];
                    if (best < 0 || a > best_a) { best = q; best_a = a; }
                }
                if (best < 0) break;
                int32_t open = 0;
                for (int q = 0; q < 4; q++)
                    if (q == best) open = k[q];
                const float* nd = nodes + 16 * (size_t)((uint32_t)open >> 2);
                const int32_t c0 = __float_as_int(nd[12]), c1 = __float_as_int(nd[13]);
                // slots indexed with constants: k stays in registers
                for (int q = 0; q < 4; q++) {
                    if (q == best) k[q] = c0;
                    if (q == nk) k[q] = c1;
                }
                nk++;
            }
            here = below[b] + (uint32_t)nk - 1u;
        }
        uint32_t mine = 0;
        for (int q = 0; q < 4; q++) mine += (q < nk && k[q] >= 0) ? 1u : 0u;
        // the wave's children in one atomic add, its largest stack bound in one atomic max
        uint32_t incl = mine, top = here;
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t v = (uint32_t)__shfl_up((int)incl, off);
            if (lane >= (uint32_t)off) incl += v;
            top = max(top, (uint32_t)__shfl_xor((int)top, off));
        }
        const uint32_t total = (uint32_t)__shfl((int)incl, 63);
        uint32_t base = 0;
        if (lane == 0) {
            if (total) base = atomicAdd(fcount + L + 1, total);
            atomicMax(res + kResWide, top);
        }
        base = (uint32_t)__shfl((int)base, 0);
        if (!act) continue;
        uint32_t at = base + incl - mine;
        for (int q = 0; q < 4; q++)
            if (q < nk && k[q] >= 0) {
                const uint32_t ch = (uint32_t)k[q] >> 2;
                dst[at++] = ch;
                below[ch] = here;
            }
        wkids[b] = make_int4(k[0], k[1], k[2], k[3]);
        flag[b] = 1u;
    }
}

__global__ __launch_bounds__(kLB) void lbvh_wide_write_kernel(uint32_t n_inner, const uint32_t* __restrict__ flag,
                                                             const uint32_t* __restrict__ widx,
                                                             const int4* __restrict__ wkids,
                                                             const float* __restrict__ nbox,
                                                             const float* __restrict__ lbox, WideNode* wide) {
    const uint32_t b = blockIdx.x * kLB + threadIdx.x;
    if (b >= n_inner || !flag[b]) return;
    const int4 kk = wkids[b];
    const int32_t k[4] = {kk.x, kk.y, kk.z, kk.w};
    const float nan = __uint_as_float(0x7fc00000u);
    float bx[6][4];
    int32_t child[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        if (k[q] == kSent) {
            for (int f = 0; f < 6; f++) bx[f][q] = nan;
            child[q] = kSent;
            continue;
        }
        const bool leaf = k[q] < 0;
        const uint32_t i = leaf ? (uint32_t)~k[q] : (uint32_t)k[q] >> 2;
        const float4* r = reinterpret_cast<const float4*>((leaf ? lbox : nbox) + 8 * (size_t)i);
        const float4 a = r[0], c = r[1];
        bx[0][q] = a.x; bx[1][q] = a.w; bx[2][q] = a.y; bx[3][q] = c.x; bx[4][q] = a.z; bx[5][q] = c.y;
        child[q] = leaf ? ~(int32_t)(i << 3 | 1u) : (int32_t)widx[i];
    }
    float4* W = reinterpret_cast<float4*>(wide + widx[b]);
    for (int f = 0; f < 6; f++) W[f] = make_float4(bx[f][0], bx[f][1], bx[f][2], bx[f][3]);
    reinterpret_cast<int4*>(W)[6] = make_int4(child[0], child[1], child[2], child[3]);
    reinterpret_cast<int4*>(W)[7] = make_int4(0, 0, 0, 0);
}

// A one-triangle mesh: node 0 with a leaf and the sentinel child (a zero box in
// the empty slot, as the host builders write it), its 4-wide copy.
__global__ void lbvh_single_kernel(const float* __restrict__ pos, float* nodes, float4* woop, uint32_t* idx,
                                   WideNode* wide, uint32_t* res) {
    f3 a, b, c;
    const TriBox tb = tri_box(pos, 0, a, b, c);
    bool bad = false;
    for (int k = 0; k < 3; k++) bad = bad || !isfinite(tb.lo[k] + tb.hi[k]) || !isfinite(tb.lo[k]) || !isfinite(tb.hi[k]);
    bad = bad || !tri_finite(a, b, c);
    res[kResFlag] = bad ? 1u : 0u;
    res[kResWide] = 1u;
    res[kResHeight] = 0u;
    for (int k = 0; k < 3; k++) { res[kResBox + k] = __float_as_uint(tb.lo[k]); res[kResBox + 3 + k] = __float_as_uint(tb.hi[k]); }
    float w[12];
    woop_set_hd(a, b, c, w);
    woop[0] = make_float4(w[0], w[1], w[2], w[3]);
    woop[1] = make_float4(w[4], w[5], w[6], w[7]);
    woop[2] = make_float4(w[8], w[9], w[10], w[11]);
    idx[0] = 1u;
    float4* F = reinterpret_cast<float4*>(nodes);
    F[0] = make_float4(tb.lo[0], tb.hi[0], tb.lo[1], tb.hi[1]);
    F[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    F[2] = make_float4(tb.lo[2], tb.hi[2], 0.0f, 0.0f);
    F[3] = make_float4(__int_as_float(~0), __int_as_float(kSent), __uint_as_float(0xffffffffu), 0.0f);
    if (wide) {
        const float nan = __uint_as_float(0x7fc00000u);
        float4* W = reinterpret_cast<float4*>(wide);
        for (int f = 0; f < 6; f++) W[f] = make_float4(f & 1 ? tb.hi[f >> 1] : tb.lo[f >> 1], nan, nan, nan);
        reinterpret_cast<int4*>(W)[6] = make_int4(~(int32_t)1, kSent, kSent, kSent);
        reinterpret_cast<int4*>(W)[7] = make_int4(0, 0, 0, 0);
    }
}

template <class T>
bool scratch_alloc(LbvhScratch* L, T** p, size_t n) { return L->pool.alloc(p, std::max<size_t>(n, 1)) == hipSuccess; }

void scratch_release(LbvhScratch* L) {
    L->pool.clear();
    L->cap = 0;
}

}  // namespace

void lbvh_free(ctl_ctx* c) {
    delete c->lbvh;
    c->lbvh = nullptr;
}

// The builder's scratch and rocPRIM's temporary storage for meshes of up to n
// triangles (kept in the context; grown after the device has drained).
int lbvh_reserve(ctl_ctx* c, uint32_t n) {
    if (!c->lbvh) c->lbvh = new LbvhScratch();
    LbvhScratch* L = c->lbvh;
    if (!L->d_res || !L->h_res) {
        if (L->d_res.grow(kLbvhResWords + kLevelWords) != hipSuccess || L->h_res.grow(kLbvhResWords) != hipSuccess) {
            c->err = "scene_rebuild_mesh: scratch allocation failed";
            return CTL_ERR_NOMEM;
        }
    }
    if (L->cap >= n) return CTL_OK;
    if (hipDeviceSynchronize() != hipSuccess) { c->err = "scene_rebuild_mesh: device synchronisation failed"; return CTL_ERR_HIP; }
    scratch_release(L);
    size_t sort_bytes = 0, scan_bytes = 0;
    if (rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr,
                                  (uint32_t*)nullptr, n, 0u, 64u, nullptr) != hipSuccess ||
        rocprim::exclusive_scan(nullptr, scan_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, n,
                                rocprim::plus<uint32_t>(), nullptr) != hipSuccess) {
        c->err = "scene_rebuild_mesh: rocPRIM storage query failed";
        return CTL_ERR_HIP;
    }
    L->tmp_bytes = std::max<size_t>(std::max(sort_bytes, scan_bytes), 16);
    const bool ok = scratch_alloc(L, &L->keys[0], n) && scratch_alloc(L, &L->keys[1], n) &&
                    scratch_alloc(L, &L->vals[0], n) && scratch_alloc(L, &L->vals[1], n) && scratch_alloc(L, &L->lpar, n) &&
                    scratch_alloc(L, &L->lbox, 8 * (size_t)n) && scratch_alloc(L, &L->nbox, 8 * (size_t)n) &&
                    scratch_alloc(L, &L->cnt, n) && scratch_alloc(L, &L->front, n) && scratch_alloc(L, &L->below, n) &&
                    scratch_alloc(L, &L->flag, n) && scratch_alloc(L, &L->widx, n) && scratch_alloc(L, &L->wkids, n) &&
                    L->pool.alloc(&L->tmp, L->tmp_bytes) == hipSuccess;
    if (!ok) {
        scratch_release(L);
        c->err = "scene_rebuild_mesh: scratch allocation failed";
        return CTL_ERR_NOMEM;
    }
    L->cap = n;
    return CTL_OK;
}

// Queues the build of n triangles into (nodes, woop, idx, wide) and the copy of
// the result words to the pinned c->lbvh->h_res; allocates nothing
// (lbvh_reserve(n) came first).  wide: null in a binary scene.
int lbvh_build(ctl_ctx* c, const float* d_pos, uint32_t n, void* nodes_, void* woop_, uint32_t* idx, void* wide_,
               hipStream_t s) {
    LbvhScratch* L = c->lbvh;
    if (!L || L->cap < n || n == 0) { c->err = "scene_rebuild_mesh: scratch not reserved"; return CTL_ERR_STATE; }
    float* nodes = static_cast<float*>(nodes_);
    float4* woop = static_cast<float4*>(woop_);
    WideNode* wide = static_cast<WideNode*>(wide_);
    uint32_t* const res = L->d_res.get();
    const dim3 blk(kLB), g_tri((n + kLB - 1) / kLB);
    auto fail = [&](const char* m) { c->err = std::string("scene_rebuild_mesh: ") + m; return (int)CTL_ERR_HIP; };
    if (n == 1) {
        hipLaunchKernelGGL(lbvh_single_kernel, dim3(1), dim3(1), 0, s, d_pos, nodes, woop, idx, wide, res);
    } else {
        const uint32_t ni = n - 1;
        const dim3 g_in((ni + kLB - 1) / kLB);
        if (hipMemsetAsync(L->cnt, 0, ni * sizeof(uint32_t), s) != hipSuccess ||
            hipMemsetAsync(L->flag, 0, ni * sizeof(uint32_t), s) != hipSuccess)
            return fail("memset failed");
        hipLaunchKernelGGL(lbvh_init_kernel, dim3(1), dim3(1), 0, s, res, L->front, L->below);
        hipLaunchKernelGGL(lbvh_box_kernel, dim3(std::min(g_tri.x, kBoxBlocks)), blk, 0, s, d_pos, n, res);
        hipLaunchKernelGGL(lbvh_key_kernel, g_tri, blk, 0, s, d_pos, n, res, L->keys[0], L->vals[0]);
        size_t tb = L->tmp_bytes;
        if (rocprim::radix_sort_pairs(L->tmp, tb, L->keys[0], L->keys[1], L->vals[0], L->vals[1], n, 0u, 64u, s) != hipSuccess)
            return fail("sort failed");
        hipLaunchKernelGGL(lbvh_tree_kernel, g_in, blk, 0, s, L->keys[1], n, nodes, L->lpar);
        hipLaunchKernelGGL(lbvh_leaf_kernel, g_tri, blk, 0, s, d_pos, L->vals[1], n, woop, idx, L->lbox);
        hipLaunchKernelGGL(lbvh_fit_kernel, g_tri, blk, 0, s, n, nodes, L->lpar, L->lbox, L->nbox, L->cnt, res);
        if (wide) {
            // level lv holds at most 4^lv nodes; the lists alternate between front and widx
            // (the scan fills widx after the last level)
            const uint32_t levels = std::min(kMaxLevels, ni);
            uint32_t* lists[2] = {L->front, L->widx};
            for (uint32_t lv = 0; lv < levels; lv++) {
                const uint64_t most = lv < 12 ? std::min<uint64_t>(1ull << (2 * lv), ni) : ni;
                const uint32_t blocks = (uint32_t)std::min<uint64_t>((most + kLB - 1) / kLB, kLevelBlocks);
                hipLaunchKernelGGL(lbvh_wide_level_kernel, dim3(blocks), blk, 0, s, lv, nodes, L->nbox, lists[lv & 1],
                                   lists[(lv + 1) & 1], L->below, L->flag, L->wkids, res);
            }
            tb = L->tmp_bytes;
            if (rocprim::exclusive_scan(L->tmp, tb, L->flag, L->widx, 0u, ni, rocprim::plus<uint32_t>(), s) != hipSuccess)
                return fail("scan failed");
            hipLaunchKernelGGL(lbvh_wide_write_kernel, g_in, blk, 0, s, ni, L->flag, L->widx, L->wkids, L->nbox, L->lbox,
                               wide);
        }
    }
    if (hipGetLastError() != hipSuccess) return fail("launch failed");
    if (hipMemcpyAsync(L->h_res.get(), res, kLbvhResWords * sizeof(uint32_t), hipMemcpyDeviceToHost, s) != hipSuccess)
        return fail("readback failed");
    return CTL_OK;
}

const uint32_t* lbvh_result(const ctl_ctx* c) { return c->lbvh ? c->lbvh->h_res.get() : nullptr; }
const uint32_t* lbvh_result_dev(const ctl_ctx* c) { return c->lbvh ? c->lbvh->d_res.get() : nullptr; }

}  // namespace ctl
