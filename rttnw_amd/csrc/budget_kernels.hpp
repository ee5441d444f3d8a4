// budget_kernels.hpp — the kernels of rttnw_budget_select and of the rounds of rttnw_render_adaptive_budget (include/rttnw_hip.h has the contract,
// DESIGN.md §10a "budgeted form" the why): the keys, a most-significant-digit radix select of the m largest of them, the mask, and the census of
// the levels a round's pixels stand at.  The arithmetic is budget_select.hpp's.  Integer atomics only: the selection is exact and does not depend
// on scheduling.  No arithmetic-namespace copies: the only value in the kernel's type is the packed mean, which is widened (as in guided_kernels.hpp).
#pragma once
#include "rt_core.hpp"
#include "budget_select.hpp"

namespace rt {

constexpr uint32_t BUDGET_BLOCK = 256u;

// What a selection leaves on the device between its launches
struct BudgetSelectState {
    BudgetKey prefix;  // the digits fixed so far, zeros below; behind the last digit: the smallest selected key
    uint32_t m;        // how many keys that match the prefix are still to be taken
    uint32_t selected; // min(candidates, max_pixels)
};

// ---- keys: the high word of every pixel's key, row-major (the low word follows from the index)
// from the row-major maps of rttnw_budget_select; `priority` (optional): the priorities themselves
__global__ void __launch_bounds__(BUDGET_BLOCK) budget_keys_maps_kernel(unsigned long long n, const double* __restrict__ value, const double* __restrict__ se,
                                                                        const uint32_t* __restrict__ spp, uint32_t cap, double rel_error, double abs_error,
                                                                        uint64_t* __restrict__ key_hi, double* __restrict__ priority) {
    for (unsigned long long q = blockIdx.x * (unsigned long long)BUDGET_BLOCK + threadIdx.x; q < n; q += gridDim.x * (unsigned long long)BUDGET_BLOCK) {
        const uint32_t s = spp[q];
        double v[3] = {0.0, 0.0, 0.0}, e[3] = {0.0, 0.0, 0.0};
        if (s != 0u) // (the colour and the error of a pixel without samples are never read)
            for (int ch = 0; ch < 3; ++ch) { v[ch] = value[q * 3ull + ch]; e[ch] = se[q * 3ull + ch]; }
        const double rho = budget_priority(v, e, s, cap, rel_error, abs_error);
        key_hi[q] = budget_key(rho, uint32_t(q)).hi;
        if (priority) priority[q] = rho;
    }
}
// from the packed means and auxiliary records of a frame that lives on one rank (adaptive_finish_packed_kernel's: the mean in the kernel's type,
// the standard errors and double(n)), as guided_raw_kernel reads them.  One thread per pixel of the image.
template <typename R>
__global__ void budget_keys_packed_kernel(const R* __restrict__ means, const double* __restrict__ aux, uint32_t width, uint32_t height, uint32_t tiles_x,
                                          uint32_t cap, double rel_error, double abs_error, uint64_t* __restrict__ key_hi) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= width || y >= height) return;
    const unsigned long long src = packed_index(x, y, tiles_x), q = (unsigned long long)y * width + x;
    const uint32_t s = uint32_t(aux[src * 4 + 3]);
    double v[3] = {0.0, 0.0, 0.0}, e[3] = {0.0, 0.0, 0.0};
    if (s != 0u)
        for (int ch = 0; ch < 3; ++ch) { v[ch] = double(means[src * 4 + ch]); e[ch] = aux[src * 4 + ch]; }
    key_hi[q] = budget_key(budget_priority(v, e, s, cap, rel_error, abs_error), uint32_t(q)).hi;
}

// ---- the radix select.  Digit d: the histogram of that digit over the candidates whose first d digits are the prefix found so far.  LDS bins per
// workgroup, then one global add per occupied bin.  (`st` is read for d > 0 only: the scan of digit 0 writes it first.)
__global__ void __launch_bounds__(BUDGET_BLOCK) budget_hist_kernel(unsigned long long n, const uint64_t* __restrict__ key_hi,
                                                                   const BudgetSelectState* __restrict__ st, uint32_t d, uint32_t* __restrict__ hist) {
    __shared__ uint32_t bins[BUDGET_BINS];
    BudgetKey prefix = {0ull, 0u};
    if (d != 0u) {
        if (st->m == 0u) return; // nothing to select: uniform over the grid
        prefix = st->prefix;
    }
    for (uint32_t i = threadIdx.x; i < BUDGET_BINS; i += BUDGET_BLOCK) bins[i] = 0u;
    __syncthreads();
    for (unsigned long long q = blockIdx.x * (unsigned long long)BUDGET_BLOCK + threadIdx.x; q < n; q += gridDim.x * (unsigned long long)BUDGET_BLOCK) {
        const BudgetKey k = {key_hi[q], 0xFFFFFFFFu - uint32_t(q)};
        if (k.hi != 0ull && budget_prefix_matches(k, prefix, d)) atomicAdd(&bins[budget_digit(k, d)], 1u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < BUDGET_BINS; i += BUDGET_BLOCK)
        if (bins[i] != 0u) atomicAdd(&hist[i], bins[i]);
}
// One workgroup walks the bins of digit d from the top: the digit in which the running count crosses m is fixed, the new prefix and what is still
// to be taken inside it stay on the device, and the bins are cleared for the next digit.  Digit 0 also settles m = min(candidates, max_pixels).
// Thread t owns BUDGET_BINS / BUDGET_BLOCK consecutive bins, the highest first.
__global__ void __launch_bounds__(BUDGET_BLOCK) budget_scan_kernel(uint32_t* __restrict__ hist, BudgetSelectState* __restrict__ st, uint32_t d,
                                                                   unsigned long long max_pixels) {
    constexpr uint32_t PER = BUDGET_BINS / BUDGET_BLOCK;
    __shared__ uint32_t sums[BUDGET_BLOCK];
    const uint32_t t = threadIdx.x;
    BudgetKey prefix = {0ull, 0u};
    uint32_t m = 0u;
    if (d != 0u) { prefix = st->prefix; m = st->m; } // (read by every thread before the first barrier, written behind the last)
    uint32_t h[PER], local = 0u;
    for (uint32_t i = 0; i < PER; ++i) {
        const uint32_t bin = BUDGET_BINS - 1u - (t * PER + i);
        h[i] = hist[bin];
        hist[bin] = 0u;
        local += h[i];
    }
    sums[t] = local;
    __syncthreads();
    for (uint32_t off = 1; off < BUDGET_BLOCK; off <<= 1) { // inclusive scan over the threads' bins
        const uint32_t add = t >= off ? sums[t - off] : 0u;
        __syncthreads();
        sums[t] += add;
        __syncthreads();
    }
    if (d == 0u) {
        const uint32_t candidates = sums[BUDGET_BLOCK - 1u];
        m = max_pixels < candidates ? uint32_t(max_pixels) : candidates;
        if (t == 0u) {
            st->selected = m;
            if (m == 0u) { st->m = 0u; st->prefix.hi = ~0ull; st->prefix.lo = ~0u; }
        }
    }
    if (m == 0u) return;
    uint32_t above = sums[t] - local; // keys in the bins above this thread's
    for (uint32_t i = 0; i < PER; ++i) {
        if (above < m && m <= above + h[i]) { // exactly one bin of one thread: the counts above it fall short of m, with it they reach m
            const BudgetKey digit = budget_digit_key(d, BUDGET_BINS - 1u - (t * PER + i));
            st->prefix.hi = prefix.hi | digit.hi;
            st->prefix.lo = prefix.lo | digit.lo;
            st->m = m - above;
        }
        above += h[i];
    }
}
// The mask: 1 for a candidate whose key is at least the threshold the scans left, else 0 — written for EVERY pixel of the image, at its row-major
// place (tiles_x == 0: rttnw_budget_select) or at its packed place on a single rank (the bytes the list compaction reads).
__global__ void __launch_bounds__(BUDGET_BLOCK) budget_mask_kernel(unsigned long long n, const uint64_t* __restrict__ key_hi,
                                                                   const BudgetSelectState* __restrict__ st, uint32_t width, uint32_t tiles_x,
                                                                   uint8_t* __restrict__ mask) {
    const bool any = st->selected != 0u;
    const BudgetKey threshold = st->prefix;
    for (unsigned long long q = blockIdx.x * (unsigned long long)BUDGET_BLOCK + threadIdx.x; q < n; q += gridDim.x * (unsigned long long)BUDGET_BLOCK) {
        const BudgetKey k = {key_hi[q], 0xFFFFFFFFu - uint32_t(q)};
        const uint8_t on = any && k.hi != 0ull && budget_key_ge(k, threshold) ? 1u : 0u;
        const unsigned long long dst = tiles_x ? packed_index(uint32_t(q % width), uint32_t(q / width), tiles_x) : q;
        mask[dst] = on;
    }
}

// ---- the census of a round: record[0] = the pixels selected, record[1 + k] = the 2x2 blocks that hold a selected pixel at level k (n == k * B),
// which is the length of the list the round's pass at level k runs over.  One thread per block of the rank.  LDS bins, BUDGET_LDS_LEVELS levels
// at a time (one sweep unless cap / B is larger), then one global add per occupied bin.
constexpr uint32_t BUDGET_LDS_LEVELS = 256u;
__global__ void __launch_bounds__(BUDGET_BLOCK) budget_census_kernel(const uint8_t* __restrict__ select, const AdaptivePixel* __restrict__ state,
                                                                     uint32_t n_blocks, uint32_t pass_spp, uint32_t n_levels,
                                                                     const BudgetSelectState* __restrict__ st, uint32_t* __restrict__ record) {
    __shared__ uint32_t bins[BUDGET_LDS_LEVELS];
    const uint32_t b = blockIdx.x * BUDGET_BLOCK + threadIdx.x;
    if (b == 0u) record[0] = st->selected;
    // the distinct levels of this block's selected pixels (a selected pixel stands below the cap: level < n_levels)
    uint32_t seen[4];
    uint32_t n_seen = 0u;
    if (b < n_blocks)
        for (uint32_t pp = 0; pp < 4u; ++pp) {
            const uint32_t p = block_pixel(b, pp);
            if (!select[p]) continue;
            const uint32_t level = state[p].n / pass_spp;
            bool is_new = level < n_levels;
            for (uint32_t i = 0; i < n_seen; ++i) is_new = is_new && seen[i] != level;
            if (is_new) seen[n_seen++] = level;
        }
    for (uint32_t base = 0; base < n_levels; base += BUDGET_LDS_LEVELS) { // (uniform over the workgroup)
        for (uint32_t i = threadIdx.x; i < BUDGET_LDS_LEVELS; i += BUDGET_BLOCK) bins[i] = 0u;
        __syncthreads();
        for (uint32_t i = 0; i < n_seen; ++i)
            if (seen[i] - base < BUDGET_LDS_LEVELS) atomicAdd(&bins[seen[i] - base], 1u); // (unsigned: a level below `base` wraps and is out)
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < BUDGET_LDS_LEVELS && base + i < n_levels; i += BUDGET_BLOCK)
            if (bins[i] != 0u) atomicAdd(&record[1u + base + i], bins[i]);
        __syncthreads();
    }
}

// ---- rttnw_render_adaptive_budget_denoised's keys (DESIGN.md §10a "filter-guided budgeted form"), between a round's filter and its selection.
// The rank: se_f = sqrt(var_f) of every pixel (+inf where the filter left nothing: its variance there is +inf), and the high word of the key
// rttnw_budget_select gives the pixel on (den, se_f, spp') — spp' = cap, "not a candidate", for a pixel that holds samples and whose OWN standard
// error is 0 in r, g and b, spp otherwise.  As in budget_keys_maps_kernel the colour and the error of a pixel without samples are never read into
// the key.  Row-major maps in, row-major keys out (the mask kernel takes them to packed places).
__global__ void __launch_bounds__(BUDGET_BLOCK) guided_budget_rank_kernel(unsigned long long n, const double* __restrict__ den, const double* __restrict__ var_f,
                                                                          const double* __restrict__ raw_stderr, const uint32_t* __restrict__ spp,
                                                                          uint32_t cap, double rel_error, double abs_error,
                                                                          double* __restrict__ stderr_f, uint64_t* __restrict__ key_hi) {
    for (unsigned long long q = blockIdx.x * (unsigned long long)BUDGET_BLOCK + threadIdx.x; q < n; q += gridDim.x * (unsigned long long)BUDGET_BLOCK) {
        const uint32_t s = spp[q];
        double v[3] = {0.0, 0.0, 0.0}, e[3] = {0.0, 0.0, 0.0};
        bool own_zero = s != 0u;
        for (int ch = 0; ch < 3; ++ch) {
            const double se = sqrt(var_f[q * 3ull + ch]);
            stderr_f[q * 3ull + ch] = se;
            if (s != 0u) {
                v[ch] = den[q * 3ull + ch];
                e[ch] = se;
                own_zero = own_zero && raw_stderr[q * 3ull + ch] == 0.0;
            }
        }
        key_hi[q] = budget_key(budget_priority(v, e, own_zero ? cap : s, cap, rel_error, abs_error), uint32_t(q)).hi;
    }
}

} // namespace rt
