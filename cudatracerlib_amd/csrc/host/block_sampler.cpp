// block_sampler.cpp — the host half of adaptive sampling: which blocks the next
// progressive pass renders (IBlockSampler::IterateBlocks) and how a finished
// pass re-ranks them (VarianceBlockSampler::AddPass,
// Kernel/BlockSampler/VarianceBlockSampler.{h,cu}; MixedBlockIterate,
// IBlockSampler.h:131-154).  No GPU: the per-block sums come from
// ctl_block_stats (image.hip), read back by the caller.
//
// Where the reference leaves the order open (std::sort, neither stable nor
// defined for NaN keys) this sampler fixes it: a NaN weight ranks below every
// number, equal weights rank by ascending block id, and every pass sorts the
// identity order afresh, so the list depends on the statistics alone.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "../../../include/ctl_trace.h"

namespace ctl { void set_host_error(const std::string& s); }

static_assert(sizeof(ctl_block_info) == 20, "VarianceBlockSampler::TmpBlockInfo is 20 B");

struct ctl_block_sampler {
    uint32_t width, height, tile, type;
    uint32_t bx, by, n;
    uint32_t frac_det = 2, frac_weighted = 4;    // KEY_FractionDeterministic / KEY_FractionWeighted
    uint32_t passes = 0;                         // m_uPassesDone: add_pass calls since start_new_rendering
    std::vector<uint32_t> order;                 // m_indices: block ids by descending weight
    std::vector<float> user, weight;             // m_userWeights; the last weights (visualizeWeights' data)
    std::vector<uint32_t> done;                  // BlockInfo::passesDone
};

namespace {

constexpr uint32_t kUniformPasses = 10;   // VarianceBlockSampler::IterateBlocks: uniform below 10 passes done

// get_w1 / get_w2 (VarianceBlockSampler.h:25-42), fp32 as the reference
float w1_of(const ctl_block_info& b) {
    if (b.num_pixels_var == 0) return 0.0f;
    return sqrtf(b.block_var_i / (float)b.num_pixels_var);
}
float w2_of(const ctl_block_info& b) {
    if (b.num_pixels_e == 0) return 0.0f;
    const float e = b.block_e_i / (float)b.num_pixels_e;
    return sqrtf(b.block_e_i2 / (float)b.num_pixels_e - e * e);
}

bool mixed(const ctl_block_sampler* s) { return s->type == CTL_BST_VARIANCE && s->passes >= kUniformPasses; }

template <class F>
void iterate(const ctl_block_sampler* s, F&& f) {
    if (!mixed(s)) {
        for (uint32_t i = 0; i < s->n; i++) f(i);
        return;
    }
    for (uint32_t i = 0; i < s->n / s->frac_weighted; i++) f(s->order[i]);
    for (uint32_t i = s->passes % s->frac_det; i < s->n; i += s->frac_det) f(i);
}

int fail(const char* m) {
    ctl::set_host_error(m);
    return CTL_ERR_INVALID;
}

}  // namespace

extern "C" {

CTL_API ctl_block_sampler* ctl_block_sampler_create(uint32_t width, uint32_t height, uint32_t tile_size,
                                                    uint32_t type) {
    if (!width || !height || !tile_size || (type != CTL_BST_UNIFORM && type != CTL_BST_VARIANCE)) {
        ctl::set_host_error("block_sampler_create: width, height and tile_size must be non-zero, type UNIFORM or VARIANCE");
        return nullptr;
    }
    const uint64_t bx = ((uint64_t)width + tile_size - 1) / tile_size, by = ((uint64_t)height + tile_size - 1) / tile_size;
    if (bx * by > 0x7fffffffull) {
        ctl::set_host_error("block_sampler_create: too many blocks");
        return nullptr;
    }
    ctl_block_sampler* s = new ctl_block_sampler();
    s->width = width; s->height = height; s->tile = tile_size; s->type = type;
    s->bx = (uint32_t)bx; s->by = (uint32_t)by; s->n = (uint32_t)(bx * by);
    s->order.resize(s->n);
    std::iota(s->order.begin(), s->order.end(), 0u);
    s->user.assign(s->n, 1.0f);
    s->weight.assign(s->n, 0.0f);
    s->done.assign(s->n, 0u);
    return s;
}

CTL_API void ctl_block_sampler_destroy(ctl_block_sampler* s) { delete s; }

CTL_API ctl_status ctl_block_sampler_start_new_rendering(ctl_block_sampler* s) {
    if (!s) return (ctl_status)fail("block_sampler: null sampler");
    s->passes = 0;
    std::iota(s->order.begin(), s->order.end(), 0u);
    std::fill(s->weight.begin(), s->weight.end(), 0.0f);
    std::fill(s->done.begin(), s->done.end(), 0u);
    return CTL_OK;
}

CTL_API ctl_status ctl_block_sampler_set_fractions(ctl_block_sampler* s, uint32_t frac_deterministic,
                                                   uint32_t frac_weighted) {
    if (!s) return (ctl_status)fail("block_sampler: null sampler");
    if (frac_deterministic < 1 || frac_weighted < 1) return (ctl_status)fail("block_sampler_set_fractions: both must be >= 1");
    s->frac_det = frac_deterministic;
    s->frac_weighted = frac_weighted;
    return CTL_OK;
}

CTL_API ctl_status ctl_block_sampler_set_user_weight(ctl_block_sampler* s, uint32_t bx, uint32_t by, float w) {
    if (!s) return (ctl_status)fail("block_sampler: null sampler");
    if (bx >= s->bx || by >= s->by) return (ctl_status)fail("block_sampler_set_user_weight: block out of range");
    s->user[(size_t)by * s->bx + bx] = w;
    return CTL_OK;
}

CTL_API ctl_status ctl_block_sampler_blocks(const ctl_block_sampler* s, uint32_t* out, uint32_t capacity, uint32_t* n) {
    if (!s || !n) return (ctl_status)fail("block_sampler_blocks: null argument");
    uint32_t cnt = 0;
    iterate(s, [&](uint32_t) { cnt++; });
    *n = cnt;
    if (capacity < cnt || (!out && cnt)) return (ctl_status)fail("block_sampler_blocks: list does not fit the capacity");
    uint32_t k = 0;
    iterate(s, [&](uint32_t b) { out[k++] = b; });
    return CTL_OK;
}

CTL_API ctl_status ctl_block_sampler_tile_samples(const ctl_block_sampler* s, uint8_t* out) {
    if (!s || !out) return (ctl_status)fail("block_sampler_tile_samples: null argument");
    std::memset(out, 0, s->n);
    iterate(s, [&](uint32_t b) { out[b]++; });   // a block is listed twice at most (once per half)
    return CTL_OK;
}

CTL_API ctl_status ctl_block_sampler_add_pass(ctl_block_sampler* s, const ctl_block_info* info, uint32_t n) {
    if (!s) return (ctl_status)fail("block_sampler: null sampler");
    if (s->type == CTL_BST_VARIANCE && (!info || n != s->n))
        return (ctl_status)fail("block_sampler_add_pass: the variance sampler needs one ctl_block_info per block");
    // what the finished pass rendered (the reference counts the next pass's list here)
    iterate(s, [&](uint32_t b) { s->done[b]++; });
    s->passes++;
    if (s->type != CTL_BST_VARIANCE) return CTL_OK;
    // min / max of both terms over all blocks; a NaN term never wins a comparison
    float min_block = FLT_MAX, max_block = -FLT_MAX, min_est = FLT_MAX, max_est = -FLT_MAX;
    for (uint32_t i = 0; i < n; i++) {
        const float est = w1_of(info[i]), blk = w2_of(info[i]);
        if (blk < min_block) min_block = blk;
        if (blk > max_block) max_block = blk;
        if (est < min_est) min_est = est;
        if (est > max_est) max_est = est;
    }
    const float lambda = 0.85f;
    for (uint32_t i = 0; i < n; i++) {   // TmpBlockInfo::getWeight x userWeight^2
        const float w1 = (w1_of(info[i]) - min_est) / (max_est - min_est);
        const float w2 = (w2_of(info[i]) - min_block) / (max_block - min_block);
        s->weight[i] = (lambda * w1 + (1 - lambda) * w2) * (s->user[i] * s->user[i]);
    }
    std::iota(s->order.begin(), s->order.end(), 0u);
    const std::vector<float>& w = s->weight;
    std::stable_sort(s->order.begin(), s->order.end(), [&](uint32_t a, uint32_t b) {
        const bool na = std::isnan(w[a]), nb = std::isnan(w[b]);
        if (na || nb) return !na && nb;
        return w[a] > w[b];
    });
    return CTL_OK;
}

CTL_API ctl_status ctl_block_sampler_weights(const ctl_block_sampler* s, float* out) {
    if (!s || !out) return (ctl_status)fail("block_sampler_weights: null argument");
    std::memcpy(out, s->weight.data(), sizeof(float) * s->n);
    return CTL_OK;
}

CTL_API ctl_status ctl_block_sampler_passes_done(const ctl_block_sampler* s, uint32_t* out) {
    if (!s || !out) return (ctl_status)fail("block_sampler_passes_done: null argument");
    std::memcpy(out, s->done.data(), sizeof(uint32_t) * s->n);
    return CTL_OK;
}

}  // extern "C"
