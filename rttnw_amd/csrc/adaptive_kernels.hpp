// adaptive_kernels.hpp — the kernels of the adaptive and region renders that compute in the render's arithmetic type, so are built once per
// arithmetic build beside the trace kernels (include/rttnw_hip.h has the contracts, DESIGN.md §10a and §10c the why): the resolve steps of a list
// pass, a rank's sums to means, its state in and out, and the window's outputs.  The steps that touch no such value — selection, marks, the list
// itself, the auxiliary maps — are built once for every precision (pixel_lists.hip).
#pragma once
#include "trace_kernels.hpp"

namespace rt {
inline namespace RT_ARITH_NS {

// ---- rttnw_render_adaptive (include/rttnw_hip.h; DESIGN.md "Adaptive sampling").
// The adaptive resolve step: resolve_kernel's chain for the pixels a pass traced, plus the pixel's noise estimate and its active bit.
// One thread per SLOT of the launch's chunk sums: pass 0 numbers them like a plain render (slot = packed pixel), a refinement pass by
// the active list (rt_core.hpp job_decode_list: slot = 4 * list position + pixel in block; `quads` != nullptr).  Per pixel, in chunk order:
// the running sum in `packed` (the R chain: exactly resolve_kernel's additions, continued over launches AND passes), and the double state
// of adaptive.hpp folded with the chunk's mean.  The pass's last launch decides whether the pixel takes part in the next pass.
// The active bit of a pixel with running sum (r, g, b) and noise state `a`: its value as the render reports it — sum / R(n), in the kernel's
// arithmetic type — held against the stopping rule.  ONE piece of code for the end of a pass (adaptive_resolve_kernel) and for a state taken up
// again (adaptive_state_import_kernel): the contracted builds' division comes from here alone, so both decide from the same bits.
template <typename R>
__device__ __forceinline__ bool adaptive_pixel_active(const AdaptivePixel& a, R r, R g, R b, double rel_error, double abs_error, uint32_t cap) {
    const R n = R(a.n);
    const double value[3] = {double(r / n), double(g / n), double(b / n)};
    return adaptive_active(a, value, rel_error, abs_error, cap);
}
template <typename R>
__global__ void adaptive_resolve_kernel(const R* __restrict__ partial, R* __restrict__ packed, AdaptivePixel* __restrict__ state,
                                        uint8_t* __restrict__ active, const uint32_t* __restrict__ quads, RenderConsts rc, uint32_t n_slots,
                                        uint32_t first_of_render, uint32_t last_of_pass, uint32_t cap, double rel_error, double abs_error) {
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= n_slots) return;
    uint32_t p = slot;
    if (quads) {
        const uint32_t e = quads[slot >> 2];
        if (((e >> QUAD_MASK_SHIFT) >> (slot & 3u) & 1u) == 0u) return; // a converged pixel of a listed block: it traced nothing
        p = block_pixel(e & QUAD_INDEX_MASK, slot & 3u);
    }
    uint32_t tx, ty;
    tile_unpermute(rc.tile_rank + (p >> 6) * rc.tile_world, rc.div_tiles_x, tx, ty);
    const bool inside = tx * 8u + (p & 7u) < rc.width && ty * 8u + ((p >> 3) & 7u) < rc.height;
    R* dst = packed + (unsigned long long)p * 4ull;
    R r = 0, g = 0, b = 0;
    AdaptivePixel a = {{0, 0, 0}, {0, 0, 0}, 0u, 0u};
    if (!first_of_render) { r = dst[0]; g = dst[1]; b = dst[2]; a = state[p]; }
    if (inside) {
        for (uint32_t c = 0; c < rc.n_chunks; ++c) {
            const R* src = partial + ((unsigned long long)c * n_slots + slot) * 3ull;
            const R sr = src[0], sg = src[1], sb = src[2];
            r = r + sr; g = g + sg; b = b + sb;
            uint32_t s0, s1;
            chunk_samples(rc, rc.chunk_base + c, s0, s1);
            const double n_c = double(s1 - s0);
            const double m[3] = {double(sr) / n_c, double(sg) / n_c, double(sb) / n_c};
            adaptive_fold(a, m, s1 - s0);
        }
    }
    dst[0] = r; dst[1] = g; dst[2] = b; dst[3] = R(0);
    state[p] = a;
    if (last_of_pass) active[p] = inside && adaptive_pixel_active<R>(a, r, g, b, rel_error, abs_error, cap) ? 1u : 0u;
}

// After the last pass: the packed running sums become the pixel means (sum / n_q, resolve_kernel's division) for untile_kernel, and the
// samples and standard errors go to row-major, top-first maps.
template <typename R>
__global__ void adaptive_output_kernel(R* __restrict__ packed, const AdaptivePixel* __restrict__ state, uint32_t* __restrict__ spp_map,
                                       double* __restrict__ stderr_map, uint32_t width, uint32_t height, uint32_t tiles_x) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= width || y >= height) return;
    const unsigned long long src = tile_permuted(x >> 3, y >> 3, tiles_x) * 64ull + ((y & 7u) << 3) + (x & 7u);
    const AdaptivePixel a = state[src];
    R* dst = packed + src * 4ull;
    const R n = R(a.n);
    dst[0] = dst[0] / n; dst[1] = dst[1] / n; dst[2] = dst[2] / n; dst[3] = R(1);
    const unsigned long long o = (unsigned long long)y * width + x;
    spp_map[o] = a.n;
    for (int ch = 0; ch < 3; ++ch) stderr_map[o * 3ull + ch] = adaptive_stderr(a, ch);
}

// ---- rttnw_render_adaptive_multi: the same step where the pixels of a frame live on several ranks.
// One rank's packed pixels after its last pass, one thread per packed pixel: the running sum becomes the mean by adaptive_output_kernel's own
// division (alpha 1), and the pixel's auxiliary record — standard error r, g, b and double(n), the shape of a packed f64 pixel, so that the gather
// moves it like one — goes to `aux`.  A pixel that traced nothing (n == 0: outside the image in an edge tile) and the pixels of pad tiles
// (p >= rank_pixels: no pass ever wrote their state) are zero-filled in both, without a division.
template <typename R>
__global__ void adaptive_finish_packed_kernel(R* __restrict__ packed, const AdaptivePixel* __restrict__ state, double* __restrict__ aux,
                                              uint32_t pixels_per_rank, uint32_t rank_pixels) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= pixels_per_rank) return;
    R* dst = packed + (unsigned long long)p * 4ull;
    double* rec = aux + (unsigned long long)p * 4ull;
    AdaptivePixel a = {{0, 0, 0}, {0, 0, 0}, 0u, 0u};
    if (p < rank_pixels) a = state[p];
    if (a.n == 0u) {
        dst[0] = R(0); dst[1] = R(0); dst[2] = R(0); dst[3] = R(0);
        rec[0] = 0.0; rec[1] = 0.0; rec[2] = 0.0; rec[3] = 0.0;
        return;
    }
    const R n = R(a.n);
    dst[0] = dst[0] / n; dst[1] = dst[1] / n; dst[2] = dst[2] / n; dst[3] = R(1);
    for (int ch = 0; ch < 3; ++ch) rec[ch] = adaptive_stderr(a, ch);
    rec[3] = double(a.n); // (n <= 2^32: exact)
}

// ---- rttnw_render_adaptive_resume: a render's state leaves the device and comes back (include/rttnw_hip.h has the record: 12 doubles per pixel —
// sum r, g, b, n, mu r, g, b, k, m2 r, g, b, 0: adaptive.hpp STATE_RECORD_DOUBLES).  The host permutes between the row-major state and a rank's packed order, so these kernels see
// one rank's packed records, one thread per packed pixel, in the single and the node-wide form alike.
// record -> running sum (narrowed back to R: exact, it was widened from R), noise state and active byte under THIS call's tolerances and cap.
// A record with n == 0 — the host leaves those for pixels outside the image and for pad tiles — gives zero state and an inactive pixel.
template <typename R>
__global__ void adaptive_state_import_kernel(const double* __restrict__ records, R* __restrict__ packed, AdaptivePixel* __restrict__ state,
                                             uint8_t* __restrict__ active, uint32_t pixels_per_rank, uint32_t cap, double rel_error, double abs_error) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= pixels_per_rank) return;
    const double* rec = records + (unsigned long long)p * STATE_RECORD_DOUBLES;
    R* dst = packed + (unsigned long long)p * 4ull;
    AdaptivePixel a = {{0, 0, 0}, {0, 0, 0}, 0u, 0u};
    R r = 0, g = 0, b = 0;
    bool on = false;
    if (rec[3] != 0.0) {
        r = R(rec[0]); g = R(rec[1]); b = R(rec[2]);
        a.n = uint32_t(rec[3]);
        a.k = uint32_t(rec[7]);
        for (int ch = 0; ch < 3; ++ch) { a.mu[ch] = rec[4 + ch]; a.m2[ch] = rec[8 + ch]; }
        on = adaptive_pixel_active<R>(a, r, g, b, rel_error, abs_error, cap);
    }
    dst[0] = r; dst[1] = g; dst[2] = b; dst[3] = R(0);
    state[p] = a;
    active[p] = on ? 1u : 0u;
}
// running sum (BEFORE adaptive_finish_packed_kernel turns it into the mean) and noise state -> record.  A pixel that traced nothing (n == 0) and
// the pixels of pad tiles (p >= rank_pixels: a fresh render never wrote their state) get a zero record.
template <typename R>
__global__ void adaptive_state_export_kernel(const R* __restrict__ packed, const AdaptivePixel* __restrict__ state, double* __restrict__ records,
                                             uint32_t pixels_per_rank, uint32_t rank_pixels) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= pixels_per_rank) return;
    double* rec = records + (unsigned long long)p * STATE_RECORD_DOUBLES;
    AdaptivePixel a = {{0, 0, 0}, {0, 0, 0}, 0u, 0u};
    if (p < rank_pixels) a = state[p];
    if (a.n == 0u) {
        for (uint32_t i = 0; i < STATE_RECORD_DOUBLES; ++i) rec[i] = 0.0;
        return;
    }
    const R* src = packed + (unsigned long long)p * 4ull;
    rec[0] = double(src[0]); rec[1] = double(src[1]); rec[2] = double(src[2]);
    rec[3] = double(a.n);
    rec[7] = double(a.k);
    for (int ch = 0; ch < 3; ++ch) { rec[4 + ch] = a.mu[ch]; rec[8 + ch] = a.m2[ch]; }
    rec[11] = 0.0;
}

// ---- rttnw_render_region around the trace kernels' active-list instantiations: the resolve step of the listed pixels and the
// window's image.  The selection and the list over it are pixel_lists.hip's.
// packed pixel p of the rank (tile * 64 + y * 8 + x) -> its pixel of the frame
__device__ __forceinline__ void packed_pixel_xy(const RenderConsts& rc, uint32_t p, uint32_t& x, uint32_t& y) {
    uint32_t tx, ty;
    tile_unpermute(rc.tile_rank + (p >> 6) * rc.tile_world, rc.div_tiles_x, tx, ty);
    x = tx * 8u + (p & 7u);
    y = ty * 8u + ((p >> 3) & 7u);
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

// ---- rttnw_render_adaptive_region (DESIGN.md §10a "windowed form"): the window's four outputs on the root.
// One thread per pixel of the window [x0, x1) x [y0, y1), untile_kernel's and untile_aux_kernel's index arithmetic on the gathered packed means
// and auxiliary records (standard error r, g, b and the sample count).  A pixel that holds samples gets its mean, RGBA8 with alpha 255, its count
// and its standard errors; one that holds none gets zeros everywhere, alpha included.  Window-sized, row-major, top row first.
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
