// region_kernels.hpp — the kernels of rttnw_render_region (include/rttnw_hip.h has the contract, DESIGN.md §10c the why) around the trace
// kernels' active-list instantiations: which pixels are selected, the resolve step of the listed pixels and the window's image.
// The list itself is built by the compaction kernels of trace_kernels.hpp (quad_count / quad_scan / quad_list) over the selection bytes.
#pragma once
#include "trace_kernels.hpp"

namespace rt {
inline namespace RT_ARITH_NS {

// packed pixel p of the rank (tile * 64 + y * 8 + x) -> its pixel of the frame
__device__ __forceinline__ void packed_pixel_xy(const RenderConsts& rc, uint32_t p, uint32_t& x, uint32_t& y) {
    uint32_t tx, ty;
    tile_unpermute(rc.tile_rank + (p >> 6) * rc.tile_world, rc.div_tiles_x, tx, ty);
    x = tx * 8u + (p & 7u);
    y = ty * 8u + ((p >> 3) & 7u);
}

// The selection byte of every packed pixel of the rank, in the order block_pixel / quad_count_kernel read: 1 for a pixel inside the window
// [x0, x1) x [y0, y1), inside the image and with a nonzero mask byte (mask: window-sized, row-major, top row first; nullptr = all), else 0.
// One thread per packed pixel; pad tiles (>= my_tiles) select nothing.
template <typename R>
__global__ void region_select_kernel(const uint8_t* __restrict__ mask, uint8_t* __restrict__ select, RenderConsts rc, uint32_t pixels_per_rank,
                                     uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= pixels_per_rank) return;
    uint8_t sel = 0;
    if (p < rc.my_tiles * 64u) {
        uint32_t x, y;
        packed_pixel_xy(rc, p, x, y);
        if (x >= x0 && x < x1 && y >= y0 && y < y1 && x < rc.width && y < rc.height)
            sel = !mask || mask[(unsigned long long)(y - y0) * (x1 - x0) + (x - x0)] ? 1u : 0u;
    }
    select[p] = sel;
}

// The resolve step over a list: resolve_kernel's chain for the selected pixels of the listed blocks.  One thread per SLOT of the launch's
// chunk sums (rt_core.hpp job_decode_list: slot = 4 * list position + pixel in block); the running sum lives in `sums`, 4 reals per slot.
// Exactly resolve_kernel's arithmetic: the launch's chunk sums added in chunk order in R onto the running sum, which the first launch
// starts and the last divides by R(spp) — so a pixel's value has the bits rttnw_render gives it.  An unselected pixel of a listed
// block traced nothing: its slot stays 0.
template <typename R>
__global__ void region_resolve_kernel(const R* __restrict__ partial, R* __restrict__ sums, const uint32_t* __restrict__ quads, uint32_t n_chunks,
                                      uint32_t n_slots, uint32_t first_launch, uint32_t last_launch, uint32_t total_spp) {
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= n_slots) return;
    R* dst = sums + (unsigned long long)slot * 4ull;
    R r = 0, g = 0, b = 0, a = 0;
    if (((quads[slot >> 2] >> QUAD_MASK_SHIFT) >> (slot & 3u) & 1u) != 0u) {
        if (!first_launch) { r = dst[0]; g = dst[1]; b = dst[2]; }
        for (uint32_t c = 0; c < n_chunks; ++c) {
            const R* src = partial + ((unsigned long long)c * n_slots + slot) * 3ull;
            r = r + src[0]; g = g + src[1]; b = b + src[2];
        }
        if (last_launch) {
            const R spp = R(total_spp);
            r = r / spp; g = g / spp; b = b / spp;
            a = R(1);
        }
    }
    dst[0] = r; dst[1] = g; dst[2] = b; dst[3] = a;
}

// The window's image: every selected pixel's mean goes from its slot to its place in the window-sized, row-major, top-first buffers, as
// untile_kernel writes a frame's (reals of R, and RGBA8 after main.rs:219-225 with alpha 255).  One thread per slot; the buffers were
// cleared beforehand, which is what an unselected pixel of the window keeps.
template <typename R>
__global__ void region_output_kernel(const R* __restrict__ sums, const uint32_t* __restrict__ quads, RenderConsts rc, uint32_t n_slots, uint32_t x0,
                                     uint32_t y0, uint32_t x1, uint32_t y1, R* __restrict__ linear_rgb, uint8_t* __restrict__ rgba8) {
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= n_slots) return;
    const uint32_t e = quads[slot >> 2];
    if (((e >> QUAD_MASK_SHIFT) >> (slot & 3u) & 1u) == 0u) return;
    uint32_t x, y;
    packed_pixel_xy(rc, block_pixel(e & QUAD_INDEX_MASK, slot & 3u), x, y);
    if (x < x0 || x >= x1 || y < y0 || y >= y1) return; // (never: region_select_kernel selects inside the window only)
    const R* src = sums + (unsigned long long)slot * 4ull;
    const R r = src[0], g = src[1], b = src[2];
    const unsigned long long o = (unsigned long long)(y - y0) * (x1 - x0) + (x - x0);
    linear_rgb[o * 3] = r; linear_rgb[o * 3 + 1] = g; linear_rgb[o * 3 + 2] = b;
    rgba8[o * 4] = quantise(r); rgba8[o * 4 + 1] = quantise(g); rgba8[o * 4 + 2] = quantise(b); rgba8[o * 4 + 3] = 255;
}

} // namespace RT_ARITH_NS
} // namespace rt
