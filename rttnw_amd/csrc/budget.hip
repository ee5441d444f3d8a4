// budget.hip — the device half of rttnw_budget_select and of the rounds of rttnw_render_adaptive_budget and rttnw_render_adaptive_budget_denoised
// (budget.hpp): the launch code of budget_kernels.hpp.  One translation unit for every precision, double only, built without -ffp-contract=fast like guided.hip and denoise.hip.
#include "budget.hpp"
#include "budget_kernels.hpp"

namespace rt {

// Workgroups of a grid-stride pass over n pixels: enough to fill the device, few enough that the bins' flush stays small beside the pass
static dim3 budget_grid(unsigned long long n) { return dim3(uint32_t(std::min<unsigned long long>((n + BUDGET_BLOCK - 1u) / BUDGET_BLOCK, 1024ull))); }

hipError_t BudgetWorkspace::alloc(unsigned long long n_pixels) {
    n = n_pixels;
    hipError_t e = key_hi.alloc(size_t(n_pixels));
    if (e == hipSuccess) e = hist.alloc(BUDGET_BINS);
    if (e == hipSuccess) e = st.alloc(sizeof(BudgetSelectState));
    if (e == hipSuccess) e = hipMemset(hist.p, 0, BUDGET_BINS * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemset(st.p, 0, sizeof(BudgetSelectState));
    return e;
}

// The select over the keys in w.key_hi: per digit a histogram pass and the one-workgroup scan that fixes the digit.  Leaves the threshold key and
// the number selected in w.st.
static void budget_select_launch(const BudgetWorkspace& w, uint64_t max_pixels, hipStream_t stream) {
    BudgetSelectState* st = (BudgetSelectState*)w.st.p;
    for (uint32_t d = 0; d < BUDGET_DIGITS; ++d) {
        hipLaunchKernelGGL(budget_hist_kernel, budget_grid(w.n), dim3(BUDGET_BLOCK), 0, stream, w.n, w.key_hi.p, st, d, w.hist.p);
        hipLaunchKernelGGL(budget_scan_kernel, dim3(1), dim3(BUDGET_BLOCK), 0, stream, w.hist.p, st, d, (unsigned long long)max_pixels);
    }
}

// What a round runs behind its keys (w.key_hi, row-major): the select of min(candidates, max_pixels) of them, the selection byte of every pixel of
// the image at its packed place, and the round's record
int budget_keys_round_launch(const BudgetWorkspace& w, const void* d_state, uint32_t width, uint32_t height, uint32_t cap, uint32_t pass_spp,
                             uint64_t max_pixels, uint8_t* d_select, uint32_t* d_record, hipStream_t stream) {
    rttnw_tile_layout L;
    fill_layout(width, height, 1, L);
    budget_select_launch(w, max_pixels, stream);
    const BudgetSelectState* st = (const BudgetSelectState*)w.st.p;
    hipLaunchKernelGGL(budget_mask_kernel, budget_grid(w.n), dim3(BUDGET_BLOCK), 0, stream, w.n, w.key_hi.p, st, width, L.tiles_x, d_select);
    const uint32_t n_blocks = L.n_tiles * 16u, n_levels = cap / pass_spp;
    HIP_TRY(hipMemsetAsync(d_record, 0, (1u + size_t(n_levels)) * sizeof(uint32_t), stream));
    hipLaunchKernelGGL(budget_census_kernel, dim3((n_blocks + BUDGET_BLOCK - 1u) / BUDGET_BLOCK), dim3(BUDGET_BLOCK), 0, stream, d_select,
                       (const AdaptivePixel*)d_state, n_blocks, pass_spp, n_levels, st, d_record);
    HIP_TRY(hipGetLastError());
    return RTTNW_OK;
}

int budget_round_launch(const BudgetWorkspace& w, uint32_t precision, const void* d_means, const double* d_aux, const void* d_state, uint32_t width,
                        uint32_t height, uint32_t cap, uint32_t pass_spp, double rel_error, double abs_error, uint64_t max_pixels, uint8_t* d_select,
                        uint32_t* d_record, hipStream_t stream) {
    rttnw_tile_layout L;
    fill_layout(width, height, 1, L);
    const dim3 block(32, 8), grid((width + 31) / 32, (height + 7) / 8);
    if (precision == RTTNW_F32)
        hipLaunchKernelGGL(budget_keys_packed_kernel<float>, grid, block, 0, stream, (const float*)d_means, d_aux, width, height, L.tiles_x, cap, rel_error,
                           abs_error, w.key_hi.p);
    else
        hipLaunchKernelGGL(budget_keys_packed_kernel<double>, grid, block, 0, stream, (const double*)d_means, d_aux, width, height, L.tiles_x, cap, rel_error,
                           abs_error, w.key_hi.p);
    return budget_keys_round_launch(w, d_state, width, height, cap, pass_spp, max_pixels, d_select, d_record, stream);
}

int guided_budget_rank_launch(const BudgetWorkspace& w, const double* d_den, const double* d_var_f, const double* d_raw_stderr, const uint32_t* d_spp,
                              uint32_t cap, double rel_error, double abs_error, double* d_stderr_f, hipStream_t stream) {
    hipLaunchKernelGGL(guided_budget_rank_kernel, budget_grid(w.n), dim3(BUDGET_BLOCK), 0, stream, w.n, d_den, d_var_f, d_raw_stderr, d_spp, cap, rel_error,
                       abs_error, d_stderr_f, w.key_hi.p);
    HIP_TRY(hipGetLastError());
    return RTTNW_OK;
}

int budget_select_device(uint32_t width, uint32_t height, const double* linear_rgb, const double* stderr_rgb, const uint32_t* spp, uint32_t cap,
                         double rel_error, double abs_error, uint64_t max_pixels, uint8_t* out_mask, double* out_priority, uint64_t* out_selected,
                         double* kernel_ms) {
    if (int rc = require_device("budget_select")) return rc;
    const char* const at = "budget_select: ";
    const unsigned long long n = (unsigned long long)width * height;
    DevBuf<double> d_value, d_se, d_priority;
    DevBuf<uint32_t> d_spp;
    DevBuf<uint8_t> d_mask;
    BudgetWorkspace w;
    HIP_TRY_AS(at, d_value.alloc(size_t(n) * 3));
    HIP_TRY_AS(at, d_se.alloc(size_t(n) * 3));
    HIP_TRY_AS(at, d_spp.alloc(size_t(n)));
    HIP_TRY_AS(at, d_mask.alloc(size_t(n)));
    if (out_priority) HIP_TRY_AS(at, d_priority.alloc(size_t(n)));
    HIP_TRY_AS(at, w.alloc(n));
    HIP_TRY_AS(at, hipMemcpy(d_value.p, linear_rgb, size_t(n) * 3 * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY_AS(at, hipMemcpy(d_se.p, stderr_rgb, size_t(n) * 3 * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY_AS(at, hipMemcpy(d_spp.p, spp, size_t(n) * sizeof(uint32_t), hipMemcpyHostToDevice));
    Event ev0, ev1;
    HIP_TRY_AS(at, create_event(ev0));
    HIP_TRY_AS(at, create_event(ev1));
    const hipStream_t stream = nullptr;
    const BudgetSelectState* st = (const BudgetSelectState*)w.st.p;
    HIP_TRY_AS(at, hipEventRecord(ev0.get(), stream));
    hipLaunchKernelGGL(budget_keys_maps_kernel, budget_grid(n), dim3(BUDGET_BLOCK), 0, stream, n, d_value.p, d_se.p, d_spp.p, cap, rel_error, abs_error,
                       w.key_hi.p, out_priority ? d_priority.p : nullptr);
    budget_select_launch(w, max_pixels, stream);
    hipLaunchKernelGGL(budget_mask_kernel, budget_grid(n), dim3(BUDGET_BLOCK), 0, stream, n, w.key_hi.p, st, width, 0u, d_mask.p);
    HIP_TRY_AS(at, hipGetLastError());
    HIP_TRY_AS(at, hipEventRecord(ev1.get(), stream));
    HIP_TRY_AS(at, hipDeviceSynchronize());
    if (kernel_ms) {
        float ms = 0;
        HIP_TRY_AS(at, hipEventElapsedTime(&ms, ev0.get(), ev1.get()));
        *kernel_ms = ms;
    }
    if (out_mask) HIP_TRY_AS(at, hipMemcpy(out_mask, d_mask.p, size_t(n), hipMemcpyDeviceToHost));
    if (out_priority) HIP_TRY_AS(at, hipMemcpy(out_priority, d_priority.p, size_t(n) * sizeof(double), hipMemcpyDeviceToHost));
    if (out_selected) {
        BudgetSelectState host;
        HIP_TRY_AS(at, hipMemcpy(&host, w.st.p, sizeof(host), hipMemcpyDeviceToHost));
        *out_selected = host.selected;
    }
    return RTTNW_OK;
}

} // namespace rt
