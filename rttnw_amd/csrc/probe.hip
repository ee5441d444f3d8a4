// probe.hip — the device half of rttnw_temporal_probe and of rttnw_svgf_set_sampling (include/rttnw_hip.h) around the arithmetic of probe.hpp.
//   probe_kernel            one thread per pixel, blocks of 64 x 4 as temporal_accumulate_kernel's: a wave is 64 consecutive pixels of one row, so its
//                           loads of this frame's planes and its stores are consecutive; the four taps of the previous frame's length, depth, alpha
//                           and normal are plain global loads, each behind its bounds test.  No colour is read.  No LDS, no atomics, no barrier.
//   probe_level_mask_kernel one thread per pixel: the byte mask {multiplier == level} that region_select_launch (pixel_lists.hip) reads
//   probe_scatter_kernel    one thread per slot of a list pass's running sums (rttnw_render_region's layout: 4 reals per slot, slot = 4 * list
//                           position + pixel in block): a selected pixel's record moves to its place in a frame's packed tiles.  A copy, no arithmetic.
#include "feature_api.hpp"
#include "filter_call.hpp"

namespace rt {
namespace {

__global__ __launch_bounds__(int(TEMPORAL_BLOCK_X* TEMPORAL_BLOCK_Y)) void probe_kernel(
    uint32_t width, uint32_t height, TemporalParams prm, SamplingParams smp, const double* __restrict__ normal, const double* __restrict__ depth,
    const double* __restrict__ alpha, const double* __restrict__ prev_length, const double* __restrict__ prev_normal,
    const double* __restrict__ prev_depth, const double* __restrict__ prev_alpha, double* __restrict__ out_length, double* __restrict__ out_prev_xy,
    uint8_t* __restrict__ out_multiplier) {
    const uint32_t x = blockIdx.x * TEMPORAL_BLOCK_X + threadIdx.x, y = blockIdx.y * TEMPORAL_BLOCK_Y + threadIdx.y;
    if (x >= width || y >= height) return;
    const ProbePixel px = probe_pixel(width, height, x, y, prm, smp, normal, depth, alpha, prev_length, prev_normal, prev_depth, prev_alpha);
    const size_t p = size_t(y) * width + x;
    out_length[p] = px.length;
    out_multiplier[p] = uint8_t(px.multiplier);
    if (out_prev_xy) {
        out_prev_xy[p * 2] = px.xy[0];
        out_prev_xy[p * 2 + 1] = px.xy[1];
    }
}

__global__ void probe_level_mask_kernel(uint32_t n, const uint8_t* __restrict__ multiplier, uint32_t level, uint8_t* __restrict__ mask) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) mask[i] = multiplier[i] == level ? 1u : 0u;
}

// R: the render's reals.  `sums` holds n_slots records of 4, `packed` the frame's tiles (tile * 64 + y * 8 + x, four reals a pixel) of rank 0 of 1:
// block b's pixel pp stands at block_pixel(b, pp), below 64 * tiles for every block the list can name.
template <typename R>
__global__ void probe_scatter_kernel(const R* __restrict__ sums, const uint32_t* __restrict__ quads, uint32_t n_slots, R* __restrict__ packed) {
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= n_slots) return;
    const uint32_t e = quads[slot >> 2];
    if (((e >> QUAD_MASK_SHIFT) >> (slot & 3u) & 1u) == 0u) return;
    const R* src = sums + size_t(slot) * 4;
    R* dst = packed + size_t(block_pixel(e & QUAD_INDEX_MASK, slot & 3u)) * 4;
    for (int k = 0; k < 4; ++k) dst[k] = src[k];
}

} // namespace

int probe_enqueue_device(const char* at, uint32_t width, uint32_t height, const TemporalParams& prm, const SamplingParams& smp, const double* d_normal,
                         const double* d_depth, const double* d_alpha, const double* d_plen, const double* d_pnormal, const double* d_pdepth,
                         const double* d_palpha, double* d_len, double* d_xy, uint8_t* d_multiplier, hipStream_t stream) {
    const dim3 block(TEMPORAL_BLOCK_X, TEMPORAL_BLOCK_Y);
    const dim3 grid((width + TEMPORAL_BLOCK_X - 1) / TEMPORAL_BLOCK_X, (height + TEMPORAL_BLOCK_Y - 1) / TEMPORAL_BLOCK_Y);
    hipLaunchKernelGGL(probe_kernel, grid, block, 0, stream, width, height, prm, smp, d_normal, d_depth, d_alpha, d_plen, d_pnormal, d_pdepth, d_palpha,
                       d_len, d_xy, d_multiplier);
    HIP_TRY_AS(at, hipGetLastError());
    return RTTNW_OK;
}

int probe_level_mask_device(const char* at, uint32_t n_pixels, const uint8_t* d_multiplier, uint32_t level, uint8_t* d_mask, hipStream_t stream) {
    hipLaunchKernelGGL(probe_level_mask_kernel, dim3((n_pixels + 255u) / 256u), dim3(256), 0, stream, n_pixels, d_multiplier, level, d_mask);
    HIP_TRY_AS(at, hipGetLastError());
    return RTTNW_OK;
}

int probe_scatter_device(const char* at, uint32_t precision, const void* d_sums, const uint32_t* d_quads, uint32_t n_quads, void* d_packed,
                         hipStream_t stream) {
    const uint32_t n_slots = n_quads * 4u;
    if (n_slots == 0) return RTTNW_OK;
    const dim3 grid((n_slots + 255u) / 256u), block(256);
    if (precision == RTTNW_F32)
        hipLaunchKernelGGL(probe_scatter_kernel<float>, grid, block, 0, stream, (const float*)d_sums, d_quads, n_slots, (float*)d_packed);
    else
        hipLaunchKernelGGL(probe_scatter_kernel<double>, grid, block, 0, stream, (const double*)d_sums, d_quads, n_slots, (double*)d_packed);
    HIP_TRY_AS(at, hipGetLastError());
    return RTTNW_OK;
}

int probe_device(uint32_t width, uint32_t height, const TemporalParams& prm, const SamplingParams& smp, const double* normal, const double* depth,
                 const double* alpha, const double* prev_length, const double* prev_normal, const double* prev_depth, const double* prev_alpha,
                 double* out_length, double* out_prev_xy, uint8_t* out_multiplier, double* kernel_ms) {
    FilterCall fc;
    if (int rc = fc.open("temporal_probe", width, height)) return rc;
    DevBuf<double> d_normal, d_depth, d_alpha, d_plen, d_pnormal, d_pdepth, d_palpha, d_len, d_xy;
    DevBuf<uint8_t> d_mult;
    fc.upload(d_normal, normal, 3);
    fc.upload(d_depth, depth, 1);
    fc.upload(d_alpha, alpha, 1);
    if (prm.has_history) {
        fc.upload(d_plen, prev_length, 1);
        fc.upload(d_pnormal, prev_normal, 3);
        fc.upload(d_pdepth, prev_depth, 1);
        fc.upload(d_palpha, prev_alpha, 1);
    }
    fc.alloc(d_len, 1);
    fc.alloc(d_xy, 2);
    fc.alloc(d_mult, 1);
    if (int rc = fc.start()) return rc;
    if (int rc = probe_enqueue_device(fc.at.c_str(), width, height, prm, smp, d_normal.p, d_depth.p, d_alpha.p, d_plen.p, d_pnormal.p, d_pdepth.p, d_palpha.p,
                                      d_len.p, d_xy.p, d_mult.p, fc.stream)) return rc;
    if (int rc = fc.finish(kernel_ms)) return rc;
    fc.copy_out(out_length, d_len, 1);
    fc.copy_out(out_prev_xy, d_xy, 2);
    fc.copy_out(out_multiplier, d_mult, 1);
    return fc.rc;
}

} // namespace rt
