// pipeline.hip — applyImagePipeline with its filters and post-process
// (Kernel/ImagePipeline/ImagePipeline.cu:54-84), arithmetic in ../ctl_image.h:
//   to_filtered_kernel      copySamplesToFiltered                    ImagePipeline.cu:23-30
//   filtered_to_rgba_kernel copyFilteredToOutput                     ImagePipeline.cu:32-41
//   filter_table_kernel +   CanonicalFilter's rtm_Copy / evalFilter  Filter/CanonicalFilter.cu:6-36
//   canonical_kernel
//   nlm_kernel              copyToCached + computeWeights +          Filter/NonLocalMeansFilter.cu:101-148,
//   nlm_apply_kernel        applyWeights                             184-229
//   lum_reduce_kernel +     Image::ComputeLuminanceInfo and          Engine/Image.cu:88-168
//   lum_final_kernel        ToneMapPostProcess::Apply's constants    PostProcess/ToneMapPostProcess.cu:26-38
//   tonemap_kernel          Reinhard05Kernel +                       ToneMapPostProcess.cu:6-24
//                           applyGammaCorrectureToOutput             ImagePipeline.cu:43-52
// fp32, reference operation order; every sum has one fixed order, so each
// output is a function of the inputs alone.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "../../../include/ctl_trace.h"
#include "common.h"
#include "../ctl_image.h"

static_assert(sizeof(ctl_image_filter) == 36, "ctl_image_filter");
static_assert(sizeof(ctl_tonemap) == 8, "ctl_tonemap");
static_assert(sizeof(ctl_luminance_info) == 28, "ctl_luminance_info");

namespace ctl {

void set_host_error(const std::string& s);   // host/scene.cpp

constexpr uint32_t kLumMaxGroups = 1024;     // luminance reduction: G = min(ceil(n / 256), 1024)
constexpr int kLumFields = 8;                // partial: sum Y, sum log, sum r, g, b, min, max, (pad)

struct LumResult {                           // written by lum_final_kernel
    ctl_luminance_info info;
    float scale, inv_wp2;                    // Reinhard05Kernel's arguments
};

struct ImageState {
    DevArray<uint32_t> d_filtered;           // filtered image when the caller passes none
    DevArray<float> d_lum;                   // kLumMaxGroups partials, then a LumResult
    DevArray<float> d_ftab;                  // canonical filter: the per-axis factors by integer distance
    // NonLocalMeansFilter's members (NonLocalMeansFilter.h:96-99)
    DevArray<float> d_weights;               // m_weightBuffer: 169 floats per pixel
    uint32_t ww = 0, wh = 0;                 // image the weights were computed for
    bool weights_valid = false;
    int64_t last_passes = -1;                // last_iter_weight_update
};

namespace {

constexpr int kR = 6, kF = 3;                        // NonLocalMeansFilter::Apply (NonLocalMeansFilter.cu:186)
constexpr int kW = 2 * kR + 1;                       // 13 offsets per axis
constexpr int kTile = 16;                            // pixels per workgroup and axis (BLOCK_SIZE)
constexpr int kHalo = kR + kF;                       // 9
constexpr int kTileW = kTile + 2 * kHalo;            // 34: colours and variances the workgroup reads
constexpr int kTermW = kTile + 2 * kF;               // 22: positions whose tap term a patch of the tile uses
static_assert(kBlock == kTile * kTile, "one thread per tile pixel");

__global__ __launch_bounds__(kBlock) void to_filtered_kernel(const ctl_pixel* fb, uint32_t n, float splat, uint32_t* out) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    out[i] = rgbe_encode(pixel_to_spectrum(fb[i], splat));
}

__global__ __launch_bounds__(kBlock) void filtered_to_rgba_kernel(const uint32_t* filtered, uint32_t n, uint32_t* out) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    out[i] = gamma_correct(rgbe_decode(filtered[i]));
}

// Reinhard05Kernel writes the linear RGBCOL; applyGammaCorrectureToOutput reads
// it back (/ 255) and quantises again after the sRGB curve.
__global__ __launch_bounds__(kBlock) void tonemap_kernel(const uint32_t* filtered, uint32_t n, const LumResult* lum,
                                                         uint32_t* out) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t lin = reinhard_pixel(filtered[i], lum->scale, lum->inv_wp2);
    out[i] = gamma_correct(from_rgbcol(lin));
}

// ---- canonical filters ------------------------------------------------------

// Filter::Evaluate(|x - _x|, |y - _y|) is a product of one factor per axis and
// the distances are integers: tab[d] = x factor of distance d < nx, tab[nx + d]
// = y factor of distance d < ny.
__global__ __launch_bounds__(kBlock) void filter_table_kernel(ctl_image_filter f, uint32_t nx, uint32_t ny, float* tab) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < nx) tab[i] = filter_factor(f, (float)i, 0);
    else if (i < nx + ny) tab[i] = filter_factor(f, (float)(i - nx), 1);
}

// window bound of evalFilter (CanonicalFilter.cu:8-11) clipped to [0, last]
__device__ __forceinline__ int64_t window_lo(float v) { v = ceilf(v); return v > 0.0f ? (int64_t)v : 0; }
__device__ __forceinline__ int64_t window_hi(float v, int64_t last) {
    v = floorf(v);
    if (!(v < 4294967296.0f)) return last;
    const int64_t i = (int64_t)v;
    return i < last ? i : last;
}

__global__ __launch_bounds__(kBlock) void canonical_kernel(const ctl_pixel* fb, uint32_t w, uint32_t h, uint32_t tiles_x,
                                                           float splat, float xw, float yw, const float* tab,
                                                           uint32_t nx, uint32_t ny, uint32_t* out) {
    const int64_t _x = (int64_t)(blockIdx.x % tiles_x) * kTile + (threadIdx.x & (kTile - 1));
    const int64_t _y = (int64_t)(blockIdx.x / tiles_x) * kTile + (threadIdx.x / kTile);
    if (_x >= w || _y >= h) return;
    const int64_t x0 = window_lo((float)_x - xw), x1 = window_hi((float)_x + xw, (int64_t)w - 1);
    const int64_t y0 = window_lo((float)_y - yw), y1 = window_hi((float)_y + yw, (int64_t)h - 1);
    spec res = mk3s(0.0f);
    if (!((x1 - x0) < 0 || (y1 - y0) < 0)) {
        spec acc = mk3s(0.0f);
        float accFilter = 0;
        for (int64_t y = y0; y <= y1; ++y) {
            const int64_t dy = y > _y ? y - _y : _y - y;
            const float fy = tab[nx + (uint32_t)(dy < ny ? dy : ny - 1)];
            for (int64_t x = x0; x <= x1; ++x) {
                const int64_t dx = x > _x ? x - _x : _x - x;
                const float filterWt = tab[(uint32_t)(dx < nx ? dx : nx - 1)] * fy;
                acc = acc + pixel_to_spectrum(fb[(size_t)y * w + x], splat) * filterWt;
                accFilter += filterWt;
            }
        }
        res = spec_div(acc, accFilter);
    }
    out[(size_t)_y * w + _x] = rgbe_encode(res);
}

// ---- non-local means --------------------------------------------------------

// The workgroup's colours as the filter sees them -- toSpectrum -> RGBE ->
// Spectrum (copyToCached, NonLocalMeansFilter.cu:150-158, then loadFromShared)
// -- and half variances times sigma2Scale in w, for the tile and a halo of
// R + F; zero outside the image (never used there).
template <int TW, int TH, int HALO, int THREADS>
__device__ __forceinline__ void nlm_fill_tile(float4* tile, const ctl_pixel* fb, const ctl_pixel_variance* var,
                                              int64_t w, int64_t h, int64_t bx0, int64_t by0, float splat,
                                              float sigma2) {
    constexpr int W = TW + 2 * HALO, H = TH + 2 * HALO;
    for (int i = threadIdx.x; i < W * H; i += THREADS) {
        const int64_t gx = bx0 - HALO + i % W, gy = by0 - HALO + i / W;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
            const size_t idx = (size_t)gy * (size_t)w + (size_t)gx;
            const spec c = rgbe_decode(rgbe_encode(pixel_to_spectrum(fb[idx], splat)));
            v = make_float4(c.x, c.y, c.z, var ? nlm_variance(var[idx], sigma2) : 0.0f);
        }
        tile[i] = v;
    }
}

__device__ __forceinline__ float tile_tap(const float4* tile, int ax, int ay, int xo, int yo, float k) {
    const float4 A = tile[ay * kTileW + ax], Q = tile[(ay + yo) * kTileW + ax + xo];
    return nlm_tap(mk3(A.x, A.y, A.z), mk3(Q.x, Q.y, Q.z), A.w, Q.w, k);
}

// computeWeights + applyWeights of one 16 x 16 tile per workgroup, offsets in
// the reference's order (xo outer, yo inner).  STORE also writes the weights
// (PixelFilterWeightBuffer's index) for later apply-only calls.
// SHARED = false is patchDistance as written: 49 taps per (p, q), each read
// from the tile and divided.  SHARED = true: a tap term depends only on the
// ordered pair (a, a + o), so for each offset o the workgroup evaluates it once
// for every a of the tile plus an apron of F into LDS, and each thread then
// adds its 7 x 7 window of terms in patchDistance's order (x outer, y inner,
// taps that leave the image with p or q skipped and not counted): the same
// fp32 values added in the same order, with 484 divisions per offset and
// workgroup instead of 12544.  The term array is double-buffered, so one
// barrier per offset separates its writers from its readers.
template <bool SHARED, bool STORE>
__global__ __launch_bounds__(kBlock) void nlm_kernel(const ctl_pixel* fb, const ctl_pixel_variance* var, uint32_t w,
                                                     uint32_t h, uint32_t tiles_x, float splat, float k, float sigma2,
                                                     float* wbuf, uint32_t* out) {
    __shared__ float4 tile[kTileW * kTileW];
    __shared__ float term[SHARED ? 2 : 1][SHARED ? kTermW * kTermW : 1];
    const int tx = threadIdx.x & (kTile - 1), ty = threadIdx.x / kTile;
    const int64_t bx0 = (int64_t)(blockIdx.x % tiles_x) * kTile, by0 = (int64_t)(blockIdx.x / tiles_x) * kTile;
    const int64_t px = bx0 + tx, py = by0 + ty;
    const bool inimg = px < w && py < h;
    const size_t pix = (size_t)py * w + (size_t)px;
    nlm_fill_tile<kTile, kTile, kHalo, kBlock>(tile, fb, var, w, h, bx0, by0, splat, sigma2);
    __syncthreads();
    spec c_p_hat = mk3s(0.0f);
    float C_p = 0;
    int oi = 0;
    for (int xo = -kR; xo <= kR; xo++)
        for (int yo = -kR; yo <= kR; yo++, oi++) {
            const float* T = term[SHARED ? (oi & 1) : 0];
            if (SHARED) {
                float* Tw = term[oi & 1];
                for (int i = threadIdx.x; i < kTermW * kTermW; i += kBlock)
                    Tw[i] = tile_tap(tile, i % kTermW + kR, i / kTermW + kR, xo, yo, k);
                __syncthreads();
            }
            const int64_t qx = px + xo, qy = py + yo;
            if (!inimg) continue;
            if (qx < 0 || qx >= w || qy < 0 || qy >= h) {
                if (STORE) wbuf[pix * (kW * kW) + (yo + kR) * kW + (xo + kR)] = 0.0f;   // ClearBuffer's value
                continue;
            }
            // the taps (x, y) with p + (x, y) and q + (x, y) inside the image
            const int64_t mx = xo < 0 ? qx : px, Mx = xo < 0 ? px : qx, my = yo < 0 ? qy : py, My = yo < 0 ? py : qy;
            const int lox = mx < kF ? -(int)mx : -kF, hix = (int64_t)w - 1 - Mx < kF ? (int)((int64_t)w - 1 - Mx) : kF;
            const int loy = my < kF ? -(int)my : -kF, hiy = (int64_t)h - 1 - My < kF ? (int)((int64_t)h - 1 - My) : kF;
            float d_range = 0, weight = 0;
            if (lox == -kF && hix == kF && loy == -kF && hiy == kF) {
#pragma unroll
                for (int x = -kF; x <= kF; x++)
#pragma unroll
                    for (int y = -kF; y <= kF; y++)
                        d_range += SHARED ? T[(ty + kF + y) * kTermW + tx + kF + x]
                                          : tile_tap(tile, tx + kHalo + x, ty + kHalo + y, xo, yo, k);
                weight = (float)((2 * kF + 1) * (2 * kF + 1));
            } else {
                for (int x = lox; x <= hix; x++)
                    for (int y = loy; y <= hiy; y++) {
                        d_range += SHARED ? T[(ty + kF + y) * kTermW + tx + kF + x]
                                          : tile_tap(tile, tx + kHalo + x, ty + kHalo + y, xo, yo, k);
                        weight++;
                    }
            }
            const float we = nlm_weight(d_range, weight);
            if (STORE) wbuf[pix * (kW * kW) + (yo + kR) * kW + (xo + kR)] = we;
            const float4 Q = tile[(ty + kHalo + yo) * kTileW + tx + kHalo + xo];
            C_p += we;
            c_p_hat = c_p_hat + mk3(Q.x, Q.y, Q.z) * we;
        }
    if (!inimg) return;
    const float4 own = tile[(ty + kHalo) * kTileW + tx + kHalo];
    out[pix] = rgbe_encode(C_p > 1e-4f ? spec_div(c_p_hat, C_p) : mk3(own.x, own.y, own.z));
}

// applyWeights (NonLocalMeansFilter.cu:117-148) with kept weights.  One wave per
// 16 x 4 pixels.  A lane's 169 weights lie 676 B from its neighbour's, but the
// 16 pixels of a tile row hold 2704 consecutive floats: the wave copies its four
// row segments into LDS with consecutive lanes on consecutive words, then each
// lane reads its own 169 from there (169 is odd, so the lanes fall on distinct
// banks).
constexpr int kApplyRows = 4, kApplyThreads = kTile * kApplyRows;
constexpr int kApplyTileW = kTile + 2 * kR, kApplyTileH = kApplyRows + 2 * kR;
__global__ __launch_bounds__(kApplyThreads) void nlm_apply_kernel(const ctl_pixel* fb, uint32_t w, uint32_t h,
                                                                 uint32_t tiles_x, float splat, const float* wbuf,
                                                                 uint32_t* out) {
    __shared__ float4 tile[kApplyTileW * kApplyTileH];
    __shared__ float wl[kApplyThreads * kW * kW];
    const int tx = threadIdx.x & (kTile - 1), ty = threadIdx.x / kTile;
    const int64_t bx0 = (int64_t)(blockIdx.x % tiles_x) * kTile, by0 = (int64_t)(blockIdx.x / tiles_x) * kApplyRows;
    const int64_t px = bx0 + tx, py = by0 + ty;
    nlm_fill_tile<kTile, kApplyRows, kR, kApplyThreads>(tile, fb, nullptr, w, h, bx0, by0, splat, 0.0f);
    const int cols = (int64_t)w - bx0 < kTile ? (int)((int64_t)w - bx0) : kTile;   // pixels of a row segment
    for (int r = 0; r < kApplyRows && by0 + r < h; r++) {
        const float* src = wbuf + ((size_t)(by0 + r) * w + (size_t)bx0) * (kW * kW);
        float* dst = wl + r * kTile * (kW * kW);
#pragma unroll 8
        for (int i = threadIdx.x; i < cols * (kW * kW); i += kApplyThreads) dst[i] = src[i];
    }
    __syncthreads();
    if (px >= w || py >= h) return;
    const size_t pix = (size_t)py * w + (size_t)px;
    const float* mine = wl + threadIdx.x * (kW * kW);
    spec c_p_hat = mk3s(0.0f);
    float C_p = 0;
    for (int xo = -kR; xo <= kR; xo++)
        for (int yo = -kR; yo <= kR; yo++) {
            const int64_t qx = px + xo, qy = py + yo;
            if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
            const float we = mine[(yo + kR) * kW + (xo + kR)];
            if (isnan(we)) continue;
            const float4 Q = tile[(ty + kR + yo) * kApplyTileW + tx + kR + xo];
            C_p += we;
            c_p_hat = c_p_hat + mk3(Q.x, Q.y, Q.z) * we;
        }
    const float4 own = tile[(ty + kR) * kApplyTileW + tx + kR];
    out[pix] = rgbe_encode(C_p > 1e-4f ? spec_div(c_p_hat, C_p) : mk3(own.x, own.y, own.z));
}

// ---- luminance --------------------------------------------------------------

// block_stats_kernel's combine (image.hip): the 64 lanes of a wave by the xor
// butterfly 32 .. 1 (every lane ends with the same bits), then thread 0 adds
// the four wave results in wave order.  s: five sums; mn / mx: minimum, maximum.
// The totals are valid in thread 0 (returns true there).
__device__ __forceinline__ bool lum_block_combine(float (&s)[5], float& mn, float& mx) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int f = 0; f < 5; f++) s[f] += __shfl_xor(s[f], off);
        mn = fminf(mn, __shfl_xor(mn, off));
        mx = fmaxf(mx, __shfl_xor(mx, off));
    }
    __shared__ float red[7][kBlock / 64];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        for (int f = 0; f < 5; f++) red[f][wave] = s[f];
        red[5][wave] = mn;
        red[6][wave] = mx;
    }
    __syncthreads();
    if (threadIdx.x != 0) return false;
    for (int f = 0; f < 5; f++) s[f] = ((red[f][0] + red[f][1]) + red[f][2]) + red[f][3];
    mn = fminf(fminf(fminf(red[5][0], red[5][1]), red[5][2]), red[5][3]);
    mx = fmaxf(fmaxf(fmaxf(red[6][0], red[6][1]), red[6][2]), red[6][3]);
    return true;
}
static_assert(kBlock == 256, "lum_block_combine adds four wave sums");

// computeLuminanceInfo's per-pixel terms (Image.cu:104-116), summed per lane
// over pixels g * 256 + t + j * G * 256, j = 0, 1, ...
__global__ __launch_bounds__(kBlock) void lum_reduce_kernel(const uint32_t* rgbe, uint32_t n, uint32_t G, float* partial) {
    float s[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    float mn = INFINITY, mx = 0.0f;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)G * kBlock) {
        const spec L_w = rgbe_decode(rgbe[i]);
        const float Y = get_luminance(L_w);
        s[0] += Y;
        s[1] += cr_log(2.3e-5f + Y);
        s[2] += L_w.x; s[3] += L_w.y; s[4] += L_w.z;
        mn = fminf(mn, Y);
        mx = fmaxf(mx, Y);
    }
    if (lum_block_combine(s, mn, mx)) {
        float* p = partial + (size_t)blockIdx.x * kLumFields;
        for (int f = 0; f < 5; f++) p[f] = s[f];
        p[5] = mn; p[6] = mx; p[7] = 0.0f;
    }
}

// The G partials combined the same way by one workgroup (lane t adds partials
// t, t + 256, ...), then ComputeLuminanceInfo's divisions (Image.cu:161-166)
// and, with tm, ToneMapPostProcess::Apply's constants.
__global__ __launch_bounds__(kBlock) void lum_final_kernel(const float* partial, uint32_t G, uint32_t w, uint32_t h,
                                                           bool tm, float key, float burn, LumResult* out) {
    float s[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    float mn = INFINITY, mx = 0.0f;
    for (uint32_t g = threadIdx.x; g < G; g += kBlock) {
        const float* p = partial + (size_t)g * kLumFields;
        for (int f = 0; f < 5; f++) s[f] += p[f];
        mn = fminf(mn, p[5]);
        mx = fmaxf(mx, p[6]);
    }
    if (!lum_block_combine(s, mn, mx)) return;
    LumResult r;
    const float n = (float)(w * h);              // avgLum /= xResolution * yResolution
    const float nc = (float)w * h;               // avgColor /= (float)xResolution * yResolution (operator/=: * 1 / f)
    const float recip = 1.0f / nc;
    r.info.min_lum = mn;
    r.info.max_lum = mx;
    r.info.avg_lum = s[0] / n;
    r.info.avg_log_lum = cr_exp(s[1] / n);
    r.info.avg_color[0] = s[2] * recip; r.info.avg_color[1] = s[3] * recip; r.info.avg_color[2] = s[4] * recip;
    r.scale = r.inv_wp2 = 0.0f;
    if (tm) tonemap_constants(key, burn, r.info.avg_log_lum, r.info.max_lum, r.scale, r.inv_wp2);
    *out = r;
}

inline uint32_t lum_groups(uint64_t n) {
    const uint64_t g = (n + kBlock - 1) / kBlock;
    return (uint32_t)(g < kLumMaxGroups ? g : kLumMaxGroups);
}

}  // namespace

void image_free(ctl_ctx* c) {
    delete c->img;
    c->img = nullptr;
}

}  // namespace ctl

using namespace ctl;

namespace {

inline unsigned blocks_of(uint64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

int image_state(ctl_ctx* c) {
    if (c->img) return CTL_OK;
    ImageState* st = new ImageState();
    if (st->d_lum.grow((size_t)kLumMaxGroups * kLumFields, sizeof(LumResult)) != hipSuccess) {
        delete st;
        c->err = "image pipeline: luminance scratch allocation failed";
        return CTL_ERR_NOMEM;
    }
    c->img = st;
    return CTL_OK;
}

// a device array that only grows (an allocation synchronises, so it happens
// only when an image is larger than any before)
template <class T>
int grow(ctl_ctx* c, DevArray<T>& a, size_t need, const char* what) {
    if (a.fits(need) || a.grow(need) == hipSuccess) return CTL_OK;
    c->err = std::string("image pipeline: ") + what + " allocation failed";
    return CTL_ERR_NOMEM;
}

LumResult* lum_result(ImageState* st) {
    return reinterpret_cast<LumResult*>(st->d_lum.get() + (size_t)kLumMaxGroups * kLumFields);
}

int launch_luminance(ctl_ctx* c, const uint32_t* rgbe, uint32_t w, uint32_t h, const ctl_tonemap* tm, hipStream_t s) {
    ImageState* st = c->img;
    const uint64_t n = (uint64_t)w * h;
    const uint32_t G = lum_groups(n);
    hipLaunchKernelGGL(lum_reduce_kernel, dim3(G), dim3(kBlock), 0, s, rgbe, (uint32_t)n, G, st->d_lum.get());
    hipLaunchKernelGGL(lum_final_kernel, dim3(1), dim3(kBlock), 0, s, (const float*)st->d_lum.get(), G, w, h, tm != nullptr,
                       tm ? tm->key : 0.0f, tm ? tm->burn : 0.0f, lum_result(st));
    CTL_HIP(c, hipGetLastError());
    return CTL_OK;
}

bool bad_width(float v) { return !(v > 0.0f) || std::isinf(v); }
bool bad_param(float v) { return !(v >= 0.0f); }

int launch_canonical(ctl_ctx* c, const ctl_pixel* fb, uint32_t w, uint32_t h, float splat, const ctl_image_filter& f,
                     uint32_t* out, hipStream_t s) {
    ImageState* st = c->img;
    // distances the window reaches: floor(width) (+ 1: the rounding of x + width), at most the image's
    auto reach = [](float width, uint32_t res) {
        const float fl = std::floor(width) + 1.0f;
        return (uint32_t)(fl < (float)(res - 1) ? fl : (float)(res - 1)) + 1u;
    };
    const uint32_t nx = reach(f.x_width, w), ny = reach(f.y_width, h);
    if (int e = grow(c, st->d_ftab, (size_t)nx + ny, "filter table")) return e;
    const uint32_t tiles_x = (w + kTile - 1) / kTile, tiles_y = (h + kTile - 1) / kTile;
    hipLaunchKernelGGL(filter_table_kernel, dim3(blocks_of((uint64_t)nx + ny)), dim3(kBlock), 0, s, f, nx, ny, st->d_ftab.get());
    hipLaunchKernelGGL(canonical_kernel, dim3(tiles_x * tiles_y), dim3(kBlock), 0, s, fb, w, h, tiles_x, splat, f.x_width,
                       f.y_width, (const float*)st->d_ftab.get(), nx, ny, out);
    CTL_HIP(c, hipGetLastError());
    return CTL_OK;
}

// NonLocalMeansFilter::Apply (NonLocalMeansFilter.cu:184-229)
int launch_nlm(ctl_ctx* c, const ctl_pixel* fb, const ctl_pixel_variance* var, uint32_t w, uint32_t h, float splat,
               uint32_t num_passes, const ctl_image_filter& f, uint32_t* out, hipStream_t s) {
    ImageState* st = c->img;
    const uint64_t n = (uint64_t)w * h;
    const uint32_t tiles_x = (w + kTile - 1) / kTile, tiles_y = (h + kTile - 1) / kTile;
    const dim3 grid(tiles_x * tiles_y), block(kBlock);
    const bool direct = (f.flags & CTL_NLM_DIRECT) != 0;
    if (f.update_periodicity == 1) {   // every call recomputes: no weight buffer, one kernel
        st->weights_valid = false;
        if (direct)
            hipLaunchKernelGGL((nlm_kernel<false, false>), grid, block, 0, s, fb, var, w, h, tiles_x, splat, f.k,
                               f.sigma2_scale, (float*)nullptr, out);
        else
            hipLaunchKernelGGL((nlm_kernel<true, false>), grid, block, 0, s, fb, var, w, h, tiles_x, splat, f.k,
                               f.sigma2_scale, (float*)nullptr, out);
    } else {
        const bool force_update = !st->weights_valid || st->ww != w || st->wh != h;
        if (force_update || st->last_passes + 1 != (int64_t)num_passes || (num_passes % f.update_periodicity) == 0) {
            st->weights_valid = false;
            if (int e = grow(c, st->d_weights, (size_t)n * (kW * kW), "NLM weight buffer")) {
                st->last_passes = -1;
                return e;
            }
            if (direct)
                hipLaunchKernelGGL((nlm_kernel<false, true>), grid, block, 0, s, fb, var, w, h, tiles_x, splat, f.k,
                                   f.sigma2_scale, st->d_weights.get(), out);
            else
                hipLaunchKernelGGL((nlm_kernel<true, true>), grid, block, 0, s, fb, var, w, h, tiles_x, splat, f.k,
                                   f.sigma2_scale, st->d_weights.get(), out);
            st->ww = w; st->wh = h;
            st->weights_valid = true;
        } else {
            const uint32_t rows = (h + kApplyRows - 1) / kApplyRows;
            hipLaunchKernelGGL(nlm_apply_kernel, dim3(tiles_x * rows), dim3(kApplyThreads), 0, s, fb, w, h, tiles_x,
                               splat, (const float*)st->d_weights.get(), out);
        }
    }
    CTL_HIP(c, hipGetLastError());
    st->last_passes = num_passes;
    return CTL_OK;
}

}  // namespace

extern "C" {

CTL_API ctl_status ctl_image_pipeline(ctl_ctx* c, const ctl_pixel* fb, const ctl_pixel_variance* var, uint32_t w,
                                      uint32_t h, float splat, uint32_t num_passes, const ctl_image_filter* filter,
                                      const ctl_tonemap* process, uint32_t* d_filtered, uint32_t* rgba, void* stream) {
    if (!c) return CTL_ERR_INVALID;
    auto refuse = [&](const char* msg) { c->err = std::string("image_pipeline: ") + msg; return (ctl_status)CTL_ERR_INVALID; };
    bool nlm = false;
    if (filter) {
        if (filter->flags & ~(uint32_t)CTL_NLM_DIRECT) return refuse("unknown flag bit");
        switch (filter->type) {
        case CTL_FILTER_BOX: case CTL_FILTER_GAUSSIAN: case CTL_FILTER_MITCHELL: case CTL_FILTER_LANCZOS:
        case CTL_FILTER_TRIANGLE:
            if (bad_width(filter->x_width) || bad_width(filter->y_width))
                return refuse("a filter width must be finite and greater than 0");
            break;
        case CTL_FILTER_NLM:
            nlm = true;
            if (filter->update_periodicity == 0) return refuse("update_periodicity must not be 0");
            if (bad_param(filter->k) || bad_param(filter->sigma2_scale))
                return refuse("k and sigma2_scale must not be negative or NaN");
            break;
        default: return refuse("unknown filter type");
        }
    }
    const uint64_t n = (uint64_t)w * h;
    if (n > 0xffffffffull) return refuse("image too large");
    if (n == 0) return CTL_OK;
    if (!fb || !rgba) return refuse("d_fb and d_rgba must not be NULL");
    if (nlm && !var) return refuse("CTL_FILTER_NLM needs d_var");
    if (!filter && !process) return ctl_image_resolve(c, fb, w, h, splat, rgba, stream);
    CTL_HIP(c, hipSetDevice(c->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (int e = image_state(c)) return e;
    ImageState* st = c->img;
    uint32_t* filtered = d_filtered;
    if (!filtered) {
        if (int e = grow(c, st->d_filtered, (size_t)n, "filtered image")) return e;
        filtered = st->d_filtered.get();
    }
    if (!filter) {
        hipLaunchKernelGGL(to_filtered_kernel, dim3(blocks_of(n)), dim3(kBlock), 0, s, fb, (uint32_t)n, splat, filtered);
        CTL_HIP(c, hipGetLastError());
    } else if (nlm) {
        if (int e = launch_nlm(c, fb, var, w, h, splat, num_passes, *filter, filtered, s)) return e;
    } else {
        if (int e = launch_canonical(c, fb, w, h, splat, *filter, filtered, s)) return e;
    }
    if (process) {
        if (int e = launch_luminance(c, filtered, w, h, process, s)) return e;
        hipLaunchKernelGGL(tonemap_kernel, dim3(blocks_of(n)), dim3(kBlock), 0, s, (const uint32_t*)filtered, (uint32_t)n,
                           (const LumResult*)lum_result(st), rgba);
    } else {
        hipLaunchKernelGGL(filtered_to_rgba_kernel, dim3(blocks_of(n)), dim3(kBlock), 0, s, (const uint32_t*)filtered,
                           (uint32_t)n, rgba);
    }
    CTL_HIP(c, hipGetLastError());
    return CTL_OK;
}

CTL_API ctl_status ctl_image_luminance(ctl_ctx* c, const uint32_t* rgbe, uint32_t w, uint32_t h,
                                       ctl_luminance_info* host_out, void* stream) {
    if (!c) return CTL_ERR_INVALID;
    if (!host_out) { c->err = "image_luminance: host_out is NULL"; return CTL_ERR_INVALID; }
    const uint64_t n = (uint64_t)w * h;
    if (n > 0xffffffffull) { c->err = "image_luminance: image too large"; return CTL_ERR_INVALID; }
    memset(host_out, 0, sizeof(*host_out));
    if (n == 0) return CTL_OK;
    if (!rgbe) { c->err = "image_luminance: d_rgbe is NULL"; return CTL_ERR_INVALID; }
    CTL_HIP(c, hipSetDevice(c->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (int e = image_state(c)) return e;
    if (int e = launch_luminance(c, rgbe, w, h, nullptr, s)) return e;
    CTL_HIP(c, hipMemcpyAsync(host_out, &lum_result(c->img)->info, sizeof(*host_out), hipMemcpyDeviceToHost, s));
    CTL_HIP(c, hipStreamSynchronize(s));
    return CTL_OK;
}

CTL_API ctl_status ctl_filter_evaluate(const ctl_image_filter* f, float x, float y, float* out) {
    if (!f || !out) { set_host_error("filter_evaluate: NULL argument"); return CTL_ERR_INVALID; }
    if (f->type < CTL_FILTER_BOX || f->type > CTL_FILTER_TRIANGLE) {
        set_host_error("filter_evaluate: not a canonical filter type");
        return CTL_ERR_INVALID;
    }
    *out = filter_evaluate(*f, x, y);
    return CTL_OK;
}

CTL_API ctl_status ctl_rgbe_encode(const float rgb[3], uint32_t* out) {
    if (!rgb || !out) { set_host_error("rgbe_encode: NULL argument"); return CTL_ERR_INVALID; }
    *out = rgbe_encode(mk3(rgb[0], rgb[1], rgb[2]));
    return CTL_OK;
}

CTL_API ctl_status ctl_rgbe_decode(uint32_t rgbe, float rgb[3]) {
    if (!rgb) { set_host_error("rgbe_decode: NULL argument"); return CTL_ERR_INVALID; }
    const spec c = rgbe_decode(rgbe);
    rgb[0] = c.x; rgb[1] = c.y; rgb[2] = c.z;
    return CTL_OK;
}

CTL_API ctl_status ctl_tonemap_constants(const ctl_tonemap* p, float avg_log_lum, float max_lum, float* scale,
                                         float* inv_wp2) {
    if (!p || !scale || !inv_wp2) { set_host_error("tonemap_constants: NULL argument"); return CTL_ERR_INVALID; }
    tonemap_constants(p->key, p->burn, avg_log_lum, max_lum, *scale, *inv_wp2);
    return CTL_OK;
}

}  // extern "C"
