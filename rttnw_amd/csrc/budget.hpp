// budget.hpp — what render_adaptive_api.cpp calls for rttnw_budget_select and for the rounds of rttnw_render_adaptive_budget and
// rttnw_render_adaptive_budget_denoised (include/rttnw_hip.h has the contracts, DESIGN.md §10a "budgeted form" and "filter-guided budgeted form" the
// why): budget.hip holds the launch code, budget_kernels.hpp the kernels, budget_select.hpp the arithmetic.  The *_launch functions enqueue on `stream` and nothing else — no allocation, no copy, no wait.
#pragma once
#include "render_common.hpp"

namespace rt {

// What a selection over n pixels keeps on the device: the high word of every key, the bins of one digit and the select's few words.
struct BudgetWorkspace {
    DevBuf<uint64_t> key_hi;
    DevBuf<uint32_t> hist;
    DevBuf<uint8_t> st;
    unsigned long long n = 0;
    hipError_t alloc(unsigned long long n_pixels); // ... and clears the bins (every select leaves them cleared)
};

// rttnw_budget_select's device half: host arrays in, host arrays out (each optional), blocking, on the current device.
int budget_select_device(uint32_t width, uint32_t height, const double* linear_rgb, const double* stderr_rgb, const uint32_t* spp, uint32_t cap,
                         double rel_error, double abs_error, uint64_t max_pixels, uint8_t* out_mask, double* out_priority, uint64_t* out_selected,
                         double* kernel_ms);

// A round's selection over a frame that lives on one rank: the keys from the packed means (reals of `precision`) and auxiliary records, the select
// of min(candidates, max_pixels) of them, the selection byte of every pixel of the image at its packed place in d_select, and d_record — 1 +
// n_levels words: the pixels selected, then per level the 2x2 blocks that hold a selected pixel standing at it (d_state: the rank's noise state).
int budget_round_launch(const BudgetWorkspace& w, uint32_t precision, const void* d_means, const double* d_aux, const void* d_state, uint32_t width,
                        uint32_t height, uint32_t cap, uint32_t pass_spp, double rel_error, double abs_error, uint64_t max_pixels, uint8_t* d_select,
                        uint32_t* d_record, hipStream_t stream);

// rttnw_render_adaptive_budget_denoised's own selection steps, over row-major maps of the frame on one device.
// Behind a round's filter: sqrt of the filtered variance of every pixel (w*h*3) and, in w.key_hi, the keys of rttnw_budget_select on (d_den, that
// root, spp') — spp' = cap for a pixel with samples whose own standard error (d_raw_stderr) is 0 in r, g and b.
int guided_budget_rank_launch(const BudgetWorkspace& w, const double* d_den, const double* d_var_f, const double* d_raw_stderr, const uint32_t* d_spp,
                              uint32_t cap, double rel_error, double abs_error, double* d_stderr_f, hipStream_t stream);
// ... and budget_round_launch's steps behind its keys, on the keys the rank left in w.key_hi: the select, d_select and d_record.
int budget_keys_round_launch(const BudgetWorkspace& w, const void* d_state, uint32_t width, uint32_t height, uint32_t cap, uint32_t pass_spp,
                             uint64_t max_pixels, uint8_t* d_select, uint32_t* d_record, hipStream_t stream);

} // namespace rt
