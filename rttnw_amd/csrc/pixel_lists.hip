// pixel_lists.hip — the kernels and the launch code of pixel_lists.hpp.  One translation unit for every precision: nothing here reads or writes
// a value of a render's arithmetic type, so it is built without the arithmetic flags of the render units (Makefile).
#include "pixel_lists.hpp"

namespace rt {

// Compaction of the marked pixels into the list of 2x2 blocks a list pass traces — deterministic, no atomics: (1) every wave counts its
// blocks with a marked pixel (ballot + popcount) and their marked pixels, (2) one workgroup scans the waves' counts, (3) every wave writes
// its entries at its base, in block order.  Block b of the rank is thread b; its entry is b | pixel mask << QUAD_MASK_SHIFT.
__device__ __forceinline__ uint32_t block_active_mask(const uint8_t* active, uint32_t b, uint32_t n_blocks) {
    uint32_t mask = 0;
    if (b < n_blocks)
        for (uint32_t pp = 0; pp < 4u; ++pp) mask |= active[block_pixel(b, pp)] ? 1u << pp : 0u;
    return mask;
}
__global__ void quad_count_kernel(const uint8_t* __restrict__ active, uint32_t n_blocks, uint32_t* __restrict__ wave_counts) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x, wave = b >> 6;
    const uint32_t mask = block_active_mask(active, b, n_blocks);
    const unsigned long long listed = __ballot(mask != 0u);
    uint32_t px = uint32_t(__popc(mask));
    for (int off = 32; off > 0; off >>= 1) px += __shfl_xor(px, off);
    if ((threadIdx.x & 63u) == 0u && wave * 64u < n_blocks) { wave_counts[2u * wave] = uint32_t(__popcll(listed)); wave_counts[2u * wave + 1u] = px; }
}
constexpr uint32_t QUAD_SCAN_BLOCK = 1024;
__global__ void __launch_bounds__(QUAD_SCAN_BLOCK) quad_scan_kernel(const uint32_t* __restrict__ wave_counts, uint32_t* __restrict__ wave_base,
                                                                    uint32_t n_waves, uint32_t* __restrict__ totals) {
    __shared__ uint32_t sq[QUAD_SCAN_BLOCK], sp[QUAD_SCAN_BLOCK];
    const uint32_t t = threadIdx.x, per = (n_waves + QUAD_SCAN_BLOCK - 1u) / QUAD_SCAN_BLOCK;
    const uint32_t w0 = t * per < n_waves ? t * per : n_waves, w1 = w0 + per < n_waves ? w0 + per : n_waves;
    uint32_t q = 0, px = 0;
    for (uint32_t w = w0; w < w1; ++w) { q += wave_counts[2u * w]; px += wave_counts[2u * w + 1u]; }
    sq[t] = q; sp[t] = px;
    __syncthreads();
    for (uint32_t off = 1; off < QUAD_SCAN_BLOCK; off <<= 1) { // inclusive scan over the threads' segments
        const uint32_t aq = t >= off ? sq[t - off] : 0u, ap = t >= off ? sp[t - off] : 0u;
        __syncthreads();
        sq[t] += aq; sp[t] += ap;
        __syncthreads();
    }
    uint32_t base = sq[t] - q;
    for (uint32_t w = w0; w < w1; ++w) { wave_base[w] = base; base += wave_counts[2u * w]; }
    if (t == QUAD_SCAN_BLOCK - 1u) { totals[0] = sq[t]; totals[1] = sp[t]; }
}
__global__ void quad_list_kernel(const uint8_t* __restrict__ active, uint32_t n_blocks, const uint32_t* __restrict__ wave_base,
                                 uint32_t* __restrict__ quads) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x, wave = b >> 6;
    const uint32_t mask = block_active_mask(active, b, n_blocks);
    const unsigned long long listed = __ballot(mask != 0u);
    if (mask) quads[wave_base[wave] + uint32_t(__popcll(listed & ((1ull << (threadIdx.x & 63u)) - 1ull)))] = b | (mask << QUAD_MASK_SHIFT);
}

// What a resumed render traces at one level: the active pixels that hold exactly level_n = level * B samples, as the byte array the list
// compaction reads.  (A fresh render has all its active pixels at one level and compacts the active bytes themselves.)
__global__ void adaptive_level_select_kernel(const uint8_t* __restrict__ active, const AdaptivePixel* __restrict__ state, uint8_t* __restrict__ marks,
                                             uint32_t n_pixels, uint32_t level_n) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pixels) return;
    marks[p] = active[p] && state[p].n == level_n ? 1u : 0u;
}

// Gathered auxiliary records (rank-major, untile_kernel's index arithmetic) -> the row-major, top-first samples and standard-error maps.
__global__ void untile_aux_kernel(const double* __restrict__ gathered_aux, uint32_t* __restrict__ spp_map, double* __restrict__ stderr_map,
                                  uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t world, uint32_t pixels_per_rank) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= width || y >= height) return;
    const uint32_t permuted = tile_permuted(x >> 3, y >> 3, tiles_x);
    const uint32_t owner = permuted % world, local_tile = permuted / world;
    const unsigned long long src = (unsigned long long)owner * pixels_per_rank + local_tile * 64ull + ((y & 7u) << 3) + (x & 7u);
    const unsigned long long o = (unsigned long long)y * width + x;
    spp_map[o] = uint32_t(gathered_aux[src * 4 + 3]);
    for (int ch = 0; ch < 3; ++ch) stderr_map[o * 3ull + ch] = gathered_aux[src * 4 + ch];
}

// The selection byte of every packed pixel of the rank, in the order block_pixel / quad_count_kernel read: 1 for a pixel inside the window
// [x0, x1) x [y0, y1), inside the image and with a nonzero mask byte (mask: window-sized, row-major, top row first; nullptr = all), else 0.
// One thread per packed pixel; pad tiles (>= my_tiles) select nothing.
__global__ void region_select_kernel(const uint8_t* __restrict__ mask, uint8_t* __restrict__ select, uint32_t width, uint32_t height, uint32_t tile_rank,
                                     uint32_t tile_world, uint32_t tiles_x, uint32_t my_tiles, uint32_t pixels_per_rank, uint32_t x0, uint32_t y0,
                                     uint32_t x1, uint32_t y1) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= pixels_per_rank) return;
    uint8_t sel = 0;
    if (p < my_tiles * 64u) {
        uint32_t tx, ty;
        tile_unpermute(tile_rank + (p >> 6) * tile_world, tiles_x, tx, ty);
        const uint32_t x = tx * 8u + (p & 7u), y = ty * 8u + ((p >> 3) & 7u);
        if (x >= x0 && x < x1 && y >= y0 && y < y1 && x < width && y < height)
            sel = !mask || mask[(unsigned long long)(y - y0) * (x1 - x0) + (x - x0)] ? 1u : 0u;
    }
    select[p] = sel;
}

// Run behind adaptive_state_import_kernel (which left every packed pixel's state, and its active byte under this call's tolerances and cap —
// 0 for a pixel without samples) and region_select_kernel (the selection byte of every packed pixel of the rank): the active byte
// rttnw_render_adaptive_region starts from.  An unselected pixel is never active; a selected pixel that holds no samples yet (n == 0: nothing to
// divide, so no stopping rule is asked) is active; a selected pixel with samples keeps the import's decision.  One thread per packed pixel.
__global__ void adaptive_region_activate_kernel(const uint8_t* __restrict__ select, const AdaptivePixel* __restrict__ state, uint8_t* __restrict__ active,
                                                uint32_t pixels_per_rank) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= pixels_per_rank) return;
    uint8_t on = 0;
    if (select[p]) on = state[p].n == 0u ? 1u : active[p];
    active[p] = on;
}

int enqueue_quad_list(const uint8_t* marks, uint32_t n_blocks, uint32_t* scan, uint32_t* quads, hipStream_t stream) {
    const uint32_t n_waves = (n_blocks + 63u) / 64u, grid = (n_blocks + 255u) / 256u;
    uint32_t* wave_counts = scan;
    uint32_t* wave_base = wave_counts + 2 * size_t(n_waves);
    uint32_t* totals = quad_list_totals(scan, n_blocks);
    hipLaunchKernelGGL(quad_count_kernel, dim3(grid), dim3(256), 0, stream, marks, n_blocks, wave_counts);
    hipLaunchKernelGGL(quad_scan_kernel, dim3(1), dim3(QUAD_SCAN_BLOCK), 0, stream, (const uint32_t*)wave_counts, wave_base, n_waves, totals);
    hipLaunchKernelGGL(quad_list_kernel, dim3(grid), dim3(256), 0, stream, marks, n_blocks, (const uint32_t*)wave_base, quads);
    HIP_TRY(hipGetLastError());
    return 0;
}

int adaptive_level_select_launch(const uint8_t* d_active, const void* d_state, uint8_t* d_marks, uint32_t n_pixels, uint32_t level_n, hipStream_t stream) {
    hipLaunchKernelGGL(adaptive_level_select_kernel, dim3((n_pixels + 255u) / 256u), dim3(256), 0, stream, d_active, (const AdaptivePixel*)d_state,
                       d_marks, n_pixels, level_n);
    HIP_TRY(hipGetLastError());
    return RTTNW_OK;
}

int untile_aux_launch(uint32_t width, uint32_t height, uint32_t world, const double* d_gathered_aux, uint32_t* d_spp, double* d_stderr, hipStream_t stream) {
    rttnw_tile_layout L;
    fill_layout(width, height, world, L);
    dim3 block(32, 8), grid((width + 31) / 32, (height + 7) / 8);
    hipLaunchKernelGGL(untile_aux_kernel, grid, block, 0, stream, d_gathered_aux, d_spp, d_stderr, width, height, L.tiles_x, world, L.pixels_per_rank);
    HIP_TRY(hipGetLastError());
    return RTTNW_OK;
}

int region_select_launch(uint32_t width, uint32_t height, uint32_t tile_rank, uint32_t tile_world, const uint8_t* d_mask, uint8_t* d_select, uint32_t x0,
                         uint32_t y0, uint32_t x1, uint32_t y1, hipStream_t stream) {
    rttnw_tile_layout L;
    fill_layout(width, height, tile_world, L);
    const uint32_t my_tiles = L.n_tiles > tile_rank ? (L.n_tiles - tile_rank + tile_world - 1) / tile_world : 0; // (base_consts' my_tiles)
    hipLaunchKernelGGL(region_select_kernel, dim3((L.pixels_per_rank + 255u) / 256u), dim3(256), 0, stream, d_mask, d_select, width, height, tile_rank,
                       tile_world, L.tiles_x, my_tiles, L.pixels_per_rank, x0, y0, x1, y1);
    HIP_TRY(hipGetLastError());
    return RTTNW_OK;
}

int adaptive_region_activate_launch(uint32_t width, uint32_t height, uint32_t tile_rank, uint32_t tile_world, const uint8_t* d_mask, uint8_t* d_select,
                                    const void* d_state, uint8_t* d_active, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, hipStream_t stream) {
    if (int rc = region_select_launch(width, height, tile_rank, tile_world, d_mask, d_select, x0, y0, x1, y1, stream)) return rc;
    rttnw_tile_layout L;
    fill_layout(width, height, tile_world, L);
    hipLaunchKernelGGL(adaptive_region_activate_kernel, dim3((L.pixels_per_rank + 255u) / 256u), dim3(256), 0, stream, (const uint8_t*)d_select,
                       (const AdaptivePixel*)d_state, d_active, L.pixels_per_rank);
    HIP_TRY(hipGetLastError());
    return RTTNW_OK;
}

} // namespace rt
