// guided_budget_kernels.hpp — the kernels rttnw_render_adaptive_budget_denoised adds (include/rttnw_hip.h has the contract, DESIGN.md §10a "filter-guided
// budgeted form" the why) between a round's filter and its selection; the kernels of the adaptive passes, of rttnw_reconstruct, of the filter-guided
// form (guided_kernels.hpp) and of the budgeted form (budget_kernels.hpp) stay untouched.  One thread per pixel of the frame, double throughout, no
// LDS and no atomics: each thread streams its pixel's six to nine doubles and writes three or four, so the kernels are bound by those bytes and a
// 256-thread workgroup of plain loads is all there is to size.  The arithmetic of the keys is budget_select.hpp's; the only value in the kernel's
// type is the packed mean, which is widened, and unfused_mul() keeps every build from fusing the one product that is followed by an add.
#pragma once
#include "budget_kernels.hpp"

namespace rt {

// guided_raw_kernel (guided_kernels.hpp) with the `valid` byte rttnw_reconstruct reads beside it: packed means and auxiliary records -> the
// row-major mean, variance = stderr * stderr (+inf with fewer than two chunks), standard error, sample count and valid = (count > 0) of every pixel.
// A pixel without samples reports zeros.
template <typename R>
__global__ void guided_budget_raw_kernel(const R* __restrict__ means, const double* __restrict__ aux, double* __restrict__ mean, double* __restrict__ variance,
                                         double* __restrict__ raw_stderr, uint32_t* __restrict__ spp, uint8_t* __restrict__ valid, uint32_t width,
                                         uint32_t height, uint32_t tiles_x) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= width || y >= height) return;
    const unsigned long long src = budget_packed_index(x, y, tiles_x), o = (unsigned long long)y * width + x;
    const uint32_t n = uint32_t(aux[src * 4 + 3]);
    for (uint32_t ch = 0; ch < 3u; ++ch) {
        const double m = n ? double(means[src * 4 + ch]) : 0.0, se = n ? aux[src * 4 + ch] : 0.0;
        mean[o * 3 + ch] = m;
        raw_stderr[o * 3 + ch] = se;
        variance[o * 3 + ch] = unfused_mul(se, se);
    }
    spp[o] = n;
    valid[o] = n ? 1u : 0u;
}

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
