// temporal.hip — the device half of rttnw_temporal_accumulate (include/rttnw_hip.h) around the arithmetic of temporal.hpp, double throughout.
//   temporal_accumulate_kernel  one thread per pixel, blocks of 64 x 4: a wave is 64 consecutive pixels of one row, so its loads of this frame's
//                               planes and its stores are consecutive doubles (24-byte records for the three-channel planes)
// The four taps of the previous frame are plain global loads: neighbouring pixels land on neighbouring history pixels, so the caches serve the
// gather, and a tile staged in LDS would have to cover wherever the block's pixels map to.  No LDS, no atomics, no barrier.
#include "feature_api.hpp"
#include "filter_call.hpp"

namespace rt {
namespace {

__global__ __launch_bounds__(int(TEMPORAL_BLOCK_X* TEMPORAL_BLOCK_Y)) void temporal_accumulate_kernel(
    uint32_t width, uint32_t height, TemporalParams prm, const double* __restrict__ linear, const double* __restrict__ variance,
    const double* __restrict__ normal, const double* __restrict__ depth, const double* __restrict__ alpha, const double* __restrict__ prev_linear,
    const double* __restrict__ prev_variance, const double* __restrict__ prev_length, const double* __restrict__ prev_normal,
    const double* __restrict__ prev_depth, const double* __restrict__ prev_alpha, double* __restrict__ out, uint8_t* __restrict__ out_rgba8,
    double* __restrict__ out_variance, double* __restrict__ out_length, double* __restrict__ out_prev_xy) {
    const uint32_t x = blockIdx.x * TEMPORAL_BLOCK_X + threadIdx.x, y = blockIdx.y * TEMPORAL_BLOCK_Y + threadIdx.y;
    if (x >= width || y >= height) return;
    const TemporalPixel px = temporal_pixel(width, height, x, y, prm, linear, variance, normal, depth, alpha, prev_linear, prev_variance, prev_length,
                                            prev_normal, prev_depth, prev_alpha);
    const size_t p = size_t(y) * width + x;
    for (int ch = 0; ch < 3; ++ch) {
        out[p * 3 + ch] = px.c[ch];
        out_rgba8[p * 4 + ch] = denoise_quantise(px.c[ch]);
        if (prm.has_variance) out_variance[p * 3 + ch] = px.v[ch];
    }
    out_rgba8[p * 4 + 3] = 255;
    out_length[p] = px.length;
    out_prev_xy[p * 2] = px.xy[0];
    out_prev_xy[p * 2 + 1] = px.xy[1];
}

} // namespace

int temporal_device(uint32_t width, uint32_t height, const TemporalParams& prm, const double* linear_rgb, const double* variance_rgb, const double* normal,
                    const double* depth, const double* alpha, const double* prev_linear_rgb, const double* prev_variance_rgb, const double* prev_length,
                    const double* prev_normal, const double* prev_depth, const double* prev_alpha, double* out_linear_rgb, uint8_t* out_rgba8,
                    double* out_variance_rgb, double* out_length, double* out_prev_xy, double* kernel_ms) {
    FilterCall fc;
    if (int rc = fc.open("temporal_accumulate", width, height)) return rc;
    const bool has_var = prm.has_variance != 0, has_history = prm.has_history != 0;
    DevBuf<double> d_lin, d_var, d_normal, d_depth, d_alpha, d_plin, d_pvar, d_plen, d_pnormal, d_pdepth, d_palpha, d_out, d_ovar, d_len, d_xy;
    DevBuf<uint8_t> d_rgba;
    fc.upload(d_lin, linear_rgb, 3);
    if (has_var) fc.upload(d_var, variance_rgb, 3);
    fc.upload(d_normal, normal, 3);
    fc.upload(d_depth, depth, 1);
    fc.upload(d_alpha, alpha, 1);
    if (has_history) {
        fc.upload(d_plin, prev_linear_rgb, 3);
        if (has_var) fc.upload(d_pvar, prev_variance_rgb, 3);
        fc.upload(d_plen, prev_length, 1);
        fc.upload(d_pnormal, prev_normal, 3);
        fc.upload(d_pdepth, prev_depth, 1);
        fc.upload(d_palpha, prev_alpha, 1);
    }
    fc.alloc(d_out, 3);
    if (has_var) fc.alloc(d_ovar, 3);
    fc.alloc(d_len, 1);
    fc.alloc(d_xy, 2);
    fc.alloc(d_rgba, 4);

    const dim3 block(TEMPORAL_BLOCK_X, TEMPORAL_BLOCK_Y);
    const dim3 grid((width + TEMPORAL_BLOCK_X - 1) / TEMPORAL_BLOCK_X, (height + TEMPORAL_BLOCK_Y - 1) / TEMPORAL_BLOCK_Y);
    if (int rc = fc.start()) return rc;
    hipLaunchKernelGGL(temporal_accumulate_kernel, grid, block, 0, fc.stream, width, height, prm, d_lin.p, d_var.p, d_normal.p, d_depth.p, d_alpha.p, d_plin.p,
                       d_pvar.p, d_plen.p, d_pnormal.p, d_pdepth.p, d_palpha.p, d_out.p, d_rgba.p, d_ovar.p, d_len.p, d_xy.p);
    HIP_TRY_AS(fc.at, hipGetLastError());
    if (int rc = fc.finish(kernel_ms)) return rc;
    fc.copy_out(out_linear_rgb, d_out, 3);
    fc.copy_out(out_rgba8, d_rgba, 4);
    if (has_var) fc.copy_out(out_variance_rgb, d_ovar, 3);
    fc.copy_out(out_length, d_len, 1);
    fc.copy_out(out_prev_xy, d_xy, 2);
    return fc.rc;
}

} // namespace rt
