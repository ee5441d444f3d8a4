// variance.hip — the device half of rttnw_temporal_variance (include/rttnw_hip.h) around the arithmetic of variance.hpp, double throughout.
//   variance_accumulate_kernel  stage A: temporal.hip's kernel with the second moment beside the colour — one thread per pixel, blocks of 64 x 4,
//                               the four taps of the previous frame plain global loads, no LDS
//   variance_estimate_kernel    stage B: one thread per pixel, blocks of 64 x 4.  A block of which some pixel takes the spatial estimate stages its
//                               pixels and a halo of the radius — (64 + 2r) x (4 + 2r) pixels, eleven planes of doubles, 76 032 bytes at radius 4
//                               — in dynamic LDS, and its short-history pixels walk their (2r + 1)^2 windows there: a wave is 64 consecutive
//                               pixels of a row and a plane's row is consecutive doubles, so every ds_read_b64 of a tap is free of bank
//                               conflicts.  The decision is one __syncthreads_or that every thread of the block reaches — uniform for the block,
//                               so for each of its waves — and the staging's own barrier sits behind it, never inside a divergent branch.  A block
//                               whose pixels all have a long history (or missed) neither stages nor waits again: in a running sequence that is
//                               most of the frame.
// No atomics.
#include "feature_api.hpp"
#include "filter_call.hpp"

namespace rt {
namespace {

__global__ __launch_bounds__(int(VARIANCE_BLOCK_X* VARIANCE_BLOCK_Y)) void variance_accumulate_kernel(
    uint32_t width, uint32_t height, TemporalParams prm, const double* __restrict__ linear, const double* __restrict__ normal,
    const double* __restrict__ depth, const double* __restrict__ alpha, const double* __restrict__ prev_linear, const double* __restrict__ prev_moment2,
    const double* __restrict__ prev_length, const double* __restrict__ prev_normal, const double* __restrict__ prev_depth,
    const double* __restrict__ prev_alpha, double* __restrict__ out, uint8_t* __restrict__ out_rgba8, double* __restrict__ out_moment2,
    double* __restrict__ out_length, double* __restrict__ out_prev_xy) {
    const uint32_t x = blockIdx.x * VARIANCE_BLOCK_X + threadIdx.x, y = blockIdx.y * VARIANCE_BLOCK_Y + threadIdx.y;
    if (x >= width || y >= height) return;
    const VarianceAccumulated px = variance_accumulate_pixel(width, height, x, y, prm, linear, normal, depth, alpha, prev_linear, prev_moment2, prev_length,
                                                             prev_normal, prev_depth, prev_alpha);
    const size_t p = size_t(y) * width + x;
    for (int ch = 0; ch < 3; ++ch) {
        out[p * 3 + ch] = px.c[ch];
        out_rgba8[p * 4 + ch] = denoise_quantise(px.c[ch]);
        out_moment2[p * 3 + ch] = px.m2[ch];
    }
    out_rgba8[p * 4 + 3] = 255;
    out_length[p] = px.length;
    out_prev_xy[p * 2] = px.xy[0];
    out_prev_xy[p * 2 + 1] = px.xy[1];
}

__global__ __launch_bounds__(int(VARIANCE_BLOCK_X* VARIANCE_BLOCK_Y)) void variance_estimate_kernel(
    uint32_t width, uint32_t height, VarianceParams prm, const double* __restrict__ m1, const double* __restrict__ m2, const double* __restrict__ length,
    const double* __restrict__ normal, const double* __restrict__ depth, const double* __restrict__ alpha, double* __restrict__ out_variance) {
    extern __shared__ __attribute__((aligned(16))) double variance_lds[];
    const int w = int(width), h = int(height), radius = int(prm.radius);
    const int x = int(blockIdx.x * VARIANCE_BLOCK_X + threadIdx.x), y = int(blockIdx.y * VARIANCE_BLOCK_Y + threadIdx.y);
    const bool inside = x < w && y < h;
    const size_t p = inside ? size_t(y) * width + size_t(x) : 0;
    const double a = inside ? alpha[p] : 0.0, n_frames = inside ? length[p] : 0.0;
    const bool spatial = inside && variance_is_spatial(prm, a, n_frames);
    double var[3];
    if (inside && !spatial) variance_temporal(a, n_frames, m1 + p * 3, m2 + p * 3, var);
    if (__syncthreads_or(spatial ? 1 : 0)) { // the same answer in every thread of the block
        const int tile_w = int(VARIANCE_BLOCK_X) + 2 * radius, tile_h = int(VARIANCE_BLOCK_Y) + 2 * radius, plane = tile_w * tile_h;
        const int tile_x0 = int(blockIdx.x * VARIANCE_BLOCK_X) - radius, tile_y0 = int(blockIdx.y * VARIANCE_BLOCK_Y) - radius;
        const int tid = int(threadIdx.y * VARIANCE_BLOCK_X + threadIdx.x);
        for (int i = tid; i < plane; i += int(VARIANCE_BLOCK_X * VARIANCE_BLOCK_Y)) {
            const int gx = tile_x0 + i % tile_w, gy = tile_y0 + i / tile_w;
            const bool in_image = gx >= 0 && gy >= 0 && gx < w && gy < h;
            const size_t g = in_image ? size_t(gy) * width + size_t(gx) : 0;
            variance_lds[i] = in_image ? alpha[g] : 0.0; // outside the image: a miss, and never read — the window tests the image's bounds itself
            variance_lds[plane + i] = in_image ? depth[g] : 0.0;
            for (int ch = 0; ch < 3; ++ch) {
                variance_lds[(2 + ch) * plane + i] = in_image ? normal[g * 3 + ch] : 0.0;
                variance_lds[(5 + ch) * plane + i] = in_image ? m1[g * 3 + ch] : 0.0;
                variance_lds[(8 + ch) * plane + i] = in_image ? m2[g * 3 + ch] : 0.0;
            }
        }
        __syncthreads();
        if (spatial) {
            const VarianceView v = {variance_lds, variance_lds + plane, variance_lds + 2 * plane, variance_lds + 5 * plane, variance_lds + 8 * plane,
                                    tile_x0,      tile_y0,              tile_w,                   1,                        plane};
            variance_spatial(v, prm, w, h, x, y, n_frames, var);
        }
    }
    if (inside)
        for (int ch = 0; ch < 3; ++ch) out_variance[p * 3 + ch] = var[ch];
}

} // namespace

// The estimate kernel's dynamic LDS, admitted once: the tile of radius 4 is more than the 64 KiB a kernel has without asking.  Before a caller starts
// its clock; rttnw_svgf_create calls it for the handle's radius.
int variance_admit_lds(const char* at, uint32_t radius) {
    HIP_TRY_AS(at, hipFuncSetAttribute(reinterpret_cast<const void*>(variance_estimate_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       int(variance_lds_bytes(radius))));
    return RTTNW_OK;
}

// The two kernels on buffers that are already on the device, enqueued on `stream` — nothing else: no allocation, no copy, no wait.  With
// prm == nullptr stage A is not run: d_out, d_m2 and d_len hold a stage A's outputs already (svgf.hip's accumulate kernel wrote them) and only the
// estimate is enqueued; d_lin, the prev_* buffers, d_rgba and d_xy are then not used.  The LDS of vprm.radius was admitted by the caller.
int variance_passes_device(const char* at, uint32_t width, uint32_t height, const TemporalParams* prm, const VarianceParams& vprm, const double* d_lin,
                           const double* d_normal, const double* d_depth, const double* d_alpha, const double* d_plin, const double* d_pm2,
                           const double* d_plen, const double* d_pnormal, const double* d_pdepth, const double* d_palpha, double* d_out, uint8_t* d_rgba,
                           double* d_m2, double* d_len, double* d_xy, double* d_var, hipStream_t stream) {
    const dim3 block(VARIANCE_BLOCK_X, VARIANCE_BLOCK_Y);
    const dim3 grid((width + VARIANCE_BLOCK_X - 1) / VARIANCE_BLOCK_X, (height + VARIANCE_BLOCK_Y - 1) / VARIANCE_BLOCK_Y);
    if (prm) {
        hipLaunchKernelGGL(variance_accumulate_kernel, grid, block, 0, stream, width, height, *prm, d_lin, d_normal, d_depth, d_alpha, d_plin, d_pm2, d_plen,
                           d_pnormal, d_pdepth, d_palpha, d_out, d_rgba, d_m2, d_len, d_xy);
        HIP_TRY_AS(at, hipGetLastError());
    }
    hipLaunchKernelGGL(variance_estimate_kernel, grid, block, variance_lds_bytes(vprm.radius), stream, width, height, vprm, d_out, d_m2, d_len, d_normal,
                       d_depth, d_alpha, d_var);
    HIP_TRY_AS(at, hipGetLastError());
    return RTTNW_OK;
}

int variance_device(uint32_t width, uint32_t height, const TemporalParams& prm, const VarianceParams& vprm, const double* linear_rgb, const double* normal,
                    const double* depth, const double* alpha, const double* prev_linear_rgb, const double* prev_moment2_rgb, const double* prev_length,
                    const double* prev_normal, const double* prev_depth, const double* prev_alpha, double* out_linear_rgb, uint8_t* out_rgba8,
                    double* out_moment2_rgb, double* out_length, double* out_prev_xy, double* out_variance_rgb, double* kernel_ms) {
    FilterCall fc;
    if (int rc = fc.open("temporal_variance", width, height)) return rc;
    MomentBuffers d;
    d.stage(fc, prm.has_history != 0, linear_rgb, normal, depth, alpha, prev_linear_rgb, prev_moment2_rgb, prev_length, prev_normal, prev_depth, prev_alpha);
    if (int rc = variance_admit_lds(fc.at.c_str(), vprm.radius)) return rc; // before the clock starts

    if (int rc = fc.start()) return rc;
    if (int rc = variance_passes_device(fc.at.c_str(), width, height, &prm, vprm, d.lin.p, d.normal.p, d.depth.p, d.alpha.p, d.plin.p, d.pm2.p, d.plen.p,
                                        d.pnormal.p, d.pdepth.p, d.palpha.p, d.out.p, d.rgba.p, d.m2.p, d.len.p, d.xy.p, d.var.p, fc.stream)) return rc;
    if (int rc = fc.finish(kernel_ms)) return rc;
    d.copy_out(fc, out_linear_rgb, out_rgba8, out_moment2_rgb, out_length, out_prev_xy, out_variance_rgb);
    return fc.rc;
}

} // namespace rt
