// adaptive_region_kernels.hpp — the kernels rttnw_render_adaptive_region adds (include/rttnw_hip.h has the contract, DESIGN.md §10a "windowed
// form" the why) to those of the resumed adaptive render and of rttnw_render_region: who of a rank's pixels is active once the state is in and
// the selection is known, and the window's four outputs on the root.  The trace, resolve, list and level kernels are the existing ones, untouched.
#pragma once
#include "region_kernels.hpp"

namespace rt {
inline namespace RT_ARITH_NS {

// Run behind adaptive_state_import_kernel (which left every packed pixel's state, and its active byte under this call's tolerances and cap —
// 0 for a pixel without samples) and region_select_kernel (the selection byte of every packed pixel of the rank): the active byte this entry
// point starts from.  An unselected pixel is never active; a selected pixel that holds no samples yet (n == 0: nothing to divide, so no
// stopping rule is asked) is active; a selected pixel with samples keeps the import's decision.  One thread per packed pixel.
template <typename R>
__global__ void adaptive_region_activate_kernel(const uint8_t* __restrict__ select, const AdaptivePixel* __restrict__ state, uint8_t* __restrict__ active,
                                                uint32_t pixels_per_rank) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= pixels_per_rank) return;
    uint8_t on = 0;
    if (select[p]) on = state[p].n == 0u ? 1u : active[p];
    active[p] = on;
}

// The window's outputs on the root: one thread per pixel of the window [x0, x1) x [y0, y1), untile_kernel's and untile_aux_kernel's index
// arithmetic on the gathered packed means and auxiliary records (standard error r, g, b and the sample count).  A pixel that holds samples
// gets its mean, RGBA8 with alpha 255, its count and its standard errors; one that holds none gets zeros everywhere, alpha included.
// Window-sized, row-major, top row first.
template <typename R>
__global__ void adaptive_region_window_kernel(const R* __restrict__ gathered, const double* __restrict__ gathered_aux, R* __restrict__ linear_rgb,
                                              uint8_t* __restrict__ rgba8, uint32_t* __restrict__ spp_map, double* __restrict__ stderr_map,
                                              uint32_t tiles_x, uint32_t world, uint32_t pixels_per_rank, uint32_t x0, uint32_t y0, uint32_t x1,
                                              uint32_t y1) {
    const uint32_t wx = blockIdx.x * blockDim.x + threadIdx.x, wy = blockIdx.y * blockDim.y + threadIdx.y;
    if (wx >= x1 - x0 || wy >= y1 - y0) return;
    const uint32_t x = x0 + wx, y = y0 + wy;
    const uint32_t permuted = tile_permuted(x >> 3, y >> 3, tiles_x);
    const uint32_t owner = permuted % world, local_tile = permuted / world;
    const unsigned long long src = (unsigned long long)owner * pixels_per_rank + local_tile * 64ull + ((y & 7u) << 3) + (x & 7u);
    const unsigned long long o = (unsigned long long)wy * (x1 - x0) + wx;
    const uint32_t n = uint32_t(gathered_aux[src * 4 + 3]);
    R r = 0, g = 0, b = 0;
    double se[3] = {0.0, 0.0, 0.0};
    if (n != 0u) {
        r = gathered[src * 4]; g = gathered[src * 4 + 1]; b = gathered[src * 4 + 2];
        for (int ch = 0; ch < 3; ++ch) se[ch] = gathered_aux[src * 4 + ch];
    }
    linear_rgb[o * 3] = r; linear_rgb[o * 3 + 1] = g; linear_rgb[o * 3 + 2] = b;
    rgba8[o * 4] = n ? quantise(r) : 0; rgba8[o * 4 + 1] = n ? quantise(g) : 0; rgba8[o * 4 + 2] = n ? quantise(b) : 0; rgba8[o * 4 + 3] = n ? 255 : 0;
    spp_map[o] = n;
    for (int ch = 0; ch < 3; ++ch) stderr_map[o * 3ull + ch] = se[ch];
}

} // namespace RT_ARITH_NS
} // namespace rt
