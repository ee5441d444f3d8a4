// guided_kernels.hpp — the kernels the filtering adaptive forms (rttnw_render_adaptive_denoised, rttnw_render_preview,
// rttnw_render_adaptive_budget_denoised; include/rttnw_hip.h has the contracts) add to those of the adaptive passes and of the filter: who
// starts alive, the raw maps the filter reads, the stopping rule behind it.  One thread per pixel of the frame, double throughout.  No arithmetic-namespace copies: the only value in the
// kernel's type is the packed mean, which is widened, and unfused_mul() keeps every build from fusing the one product that is followed by an add.
#pragma once
#include "rt_core.hpp"
#include "denoise.hpp"

namespace rt {

// Before round 0, the alive byte of every packed pixel of the image: 1 on the lattice x % 2^level == 0 && y % 2^level == 0 (level 0: every
// pixel — rttnw_render_adaptive_denoised; rttnw_render_preview picks the level), 0 elsewhere (the buffer was cleared: the rest of an edge tile stays 0)
__global__ void guided_lattice_kernel(uint8_t* __restrict__ alive, uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t level) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= width || y >= height) return;
    const uint32_t low = (1u << level) - 1u;
    alive[packed_index(x, y, tiles_x)] = ((x | y) & low) == 0u ? 1u : 0u;
}

// Packed means and auxiliary records -> the row-major mean, variance, standard error and sample count of every pixel, stopped ones with their
// frozen values, and — where the caller has a use for it (`valid` != nullptr) — the byte rttnw_reconstruct reads beside them: valid = (count > 0).
// variance = stderr * stderr (+inf with fewer than two chunks).  A pixel without samples reports zeros, as the windowed form does.
template <typename R>
__global__ void guided_raw_kernel(const R* __restrict__ means, const double* __restrict__ aux, double* __restrict__ mean, double* __restrict__ variance,
                                  double* __restrict__ raw_stderr, uint32_t* __restrict__ spp, uint8_t* __restrict__ valid, uint32_t width, uint32_t height,
                                  uint32_t tiles_x) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= width || y >= height) return;
    const unsigned long long src = packed_index(x, y, tiles_x), o = (unsigned long long)y * width + x;
    const uint32_t n = uint32_t(aux[src * 4 + 3]);
    for (uint32_t ch = 0; ch < 3u; ++ch) {
        const double m = n ? double(means[src * 4 + ch]) : 0.0, se = n ? aux[src * 4 + ch] : 0.0;
        mean[o * 3 + ch] = m;
        raw_stderr[o * 3 + ch] = se;
        variance[o * 3 + ch] = unfused_mul(se, se);
    }
    spp[o] = n;
    if (valid) valid[o] = n ? 1u : 0u;
}

// The stopping rule on the filtered image: an alive pixel stops, for good, if its own standard error is 0 in r, g and b, or if for each of r, g, b
// the filtered variance is finite and sqrt(var_f) <= abs_error + rel_error * den.  Writes the packed alive bytes the list compaction reads
// (quad_count_kernel / quad_list_kernel: they are the next round's active AND selection bytes), and sqrt(var_f) for every pixel of the frame.
__global__ void guided_stop_kernel(const double* __restrict__ den, const double* __restrict__ var_f, const double* __restrict__ raw_stderr,
                                   double rel_error, double abs_error, uint8_t* __restrict__ alive, double* __restrict__ stderr_f, uint32_t width,
                                   uint32_t height, uint32_t tiles_x) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= width || y >= height) return;
    const unsigned long long src = packed_index(x, y, tiles_x), o = (unsigned long long)y * width + x;
    bool own_zero = true, filtered = true;
    for (uint32_t ch = 0; ch < 3u; ++ch) {
        const double v = var_f[o * 3 + ch], se = sqrt(v);
        stderr_f[o * 3 + ch] = se;
        own_zero = own_zero && raw_stderr[o * 3 + ch] == 0.0;
        filtered = filtered && denoise_finite(v) && se <= abs_error + unfused_mul(rel_error, den[o * 3 + ch]);
    }
    if (alive[src] && (own_zero || filtered)) alive[src] = 0u;
}

} // namespace rt
