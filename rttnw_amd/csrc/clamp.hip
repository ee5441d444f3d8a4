// clamp.hip — the device half of rttnw_temporal_clamp and of the clamped rttnw_svgf handle (include/rttnw_hip.h) around the arithmetic of
// clamp.hpp, double throughout.
//   clamp_accumulate_kernel  stages S and A' fused: one thread per pixel, blocks of 64 x 4 like temporal.hip's.  A thread does its reprojection
//                            and four taps from global memory, as svgf_accumulate_kernel does — M1, M2 and, with feedback, H on them.  The block
//                            then votes once, with a __syncthreads_or that every thread reaches: did any of its pixels get W > 0 (or were the
//                            statistics asked for and a pixel hit)?  Only then it stages its pixels and a halo of the radius — (64 + 2r) x (4 + 2r)
//                            pixels, eight planes of doubles (alpha, depth, normal, this frame's colour), 44 800 bytes at radius 3, 55 296 at
//                            radius 4, under the 64 KiB a kernel has without asking — in dynamic LDS, and the threads that need bounds walk their
//                            (2r + 1)^2 windows there: a wave is 64 consecutive pixels of a row and a plane's row is consecutive doubles, so every
//                            ds_read_b64 of a tap is free of bank conflicts; colour * colour is formed per tap.  Then the clip and the blend.  The
//                            staging's barrier sits behind the uniform vote, never inside a divergent branch; a first frame, or a block of
//                            misses, stages nothing and does not wait again.
// Stage B is variance.hip's estimate kernel, as it is, over this kernel's outputs.  No atomics.
#include "feature_api.hpp"
#include "filter_call.hpp"

namespace rt {
namespace {

__global__ __launch_bounds__(int(CLAMP_BLOCK_X* CLAMP_BLOCK_Y)) void clamp_accumulate_kernel(
    uint32_t width, uint32_t height, TemporalParams prm, ClampParams kprm, uint32_t feedback, const double* __restrict__ linear,
    const double* __restrict__ normal, const double* __restrict__ depth, const double* __restrict__ alpha, const double* __restrict__ prev_moment1,
    const double* __restrict__ prev_moment2, const double* __restrict__ prev_history, const double* __restrict__ prev_length,
    const double* __restrict__ prev_normal, const double* __restrict__ prev_depth, const double* __restrict__ prev_alpha, double* __restrict__ out_moment1,
    uint8_t* __restrict__ out_rgba8, double* __restrict__ out_moment2, double* __restrict__ out_acc, double* __restrict__ out_length,
    double* __restrict__ out_prev_xy, double* __restrict__ out_mean, double* __restrict__ out_sd, uint8_t* __restrict__ out_clipped) {
    extern __shared__ __attribute__((aligned(16))) double clamp_lds[];
    const int w = int(width), h = int(height), radius = int(kprm.radius);
    const int x = int(blockIdx.x * CLAMP_BLOCK_X + threadIdx.x), y = int(blockIdx.y * CLAMP_BLOCK_Y + threadIdx.y);
    const bool inside = x < w && y < h;
    const size_t p = inside ? size_t(y) * width + size_t(x) : 0;
    const bool want_stats = out_mean != nullptr || out_sd != nullptr;
    ClampGathered g;
    g.blend = false;
    double cur[3] = {0.0, 0.0, 0.0}, mu[3], sd[3];
    bool hit = false;
    if (inside) {
        g = clamp_gather_pixel(width, height, uint32_t(x), uint32_t(y), prm, feedback != 0u, normal, depth, alpha, prev_moment1, prev_moment2, prev_history,
                               prev_length, prev_normal, prev_depth, prev_alpha);
        hit = alpha[p] != 0.0;
        for (int ch = 0; ch < 3; ++ch) {
            cur[ch] = linear[p * 3 + ch];
            mu[ch] = cur[ch]; // a miss's, and what nobody reads where no bounds are needed
            sd[ch] = 0.0;
        }
    }
    const bool walks = inside && (g.blend || (want_stats && hit));
    if (__syncthreads_or(walks ? 1 : 0)) { // the same answer in every thread of the block
        const int tile_w = int(CLAMP_BLOCK_X) + 2 * radius, tile_h = int(CLAMP_BLOCK_Y) + 2 * radius, plane = tile_w * tile_h;
        const int tile_x0 = int(blockIdx.x * CLAMP_BLOCK_X) - radius, tile_y0 = int(blockIdx.y * CLAMP_BLOCK_Y) - radius;
        const int tid = int(threadIdx.y * CLAMP_BLOCK_X + threadIdx.x);
        for (int i = tid; i < plane; i += int(CLAMP_BLOCK_X * CLAMP_BLOCK_Y)) {
            const int gx = tile_x0 + i % tile_w, gy = tile_y0 + i / tile_w;
            const bool in_image = gx >= 0 && gy >= 0 && gx < w && gy < h;
            const size_t q = in_image ? size_t(gy) * width + size_t(gx) : 0;
            clamp_lds[i] = in_image ? alpha[q] : 0.0; // outside the image: a miss, and never read — the window tests the image's bounds itself
            clamp_lds[plane + i] = in_image ? depth[q] : 0.0;
            for (int ch = 0; ch < 3; ++ch) {
                clamp_lds[(2 + ch) * plane + i] = in_image ? normal[q * 3 + ch] : 0.0;
                clamp_lds[(5 + ch) * plane + i] = in_image ? linear[q * 3 + ch] : 0.0;
            }
        }
        __syncthreads();
        if (walks) {
            const ClampView v = {clamp_lds, clamp_lds + plane, clamp_lds + 2 * plane, clamp_lds + 5 * plane, tile_x0, tile_y0, tile_w, 1, plane};
            clamp_statistics(v, kprm, w, h, x, y, mu, sd);
        }
    }
    if (!inside) return;
    const ClampAccumulated px = clamp_finish_pixel(g, prm, kprm, feedback != 0u, cur, mu, sd);
    for (int ch = 0; ch < 3; ++ch) {
        out_moment1[p * 3 + ch] = px.m1[ch];
        out_moment2[p * 3 + ch] = px.m2[ch];
        if (out_rgba8) out_rgba8[p * 4 + ch] = denoise_quantise(px.m1[ch]);
        if (out_acc) out_acc[p * 3 + ch] = px.a[ch];
        if (out_mean) out_mean[p * 3 + ch] = mu[ch];
        if (out_sd) out_sd[p * 3 + ch] = sd[ch];
    }
    if (out_rgba8) out_rgba8[p * 4 + 3] = 255;
    out_length[p] = px.length;
    out_prev_xy[p * 2] = g.xy[0];
    out_prev_xy[p * 2 + 1] = g.xy[1];
    out_clipped[p] = px.clipped;
}

} // namespace

// Stages S and A' on buffers that are already on the device, enqueued on `stream` — nothing else: no allocation, no copy, no wait.  d_phist: the
// fed-back colour history (the rttnw_svgf handle's, read with `feedback`), or nullptr; d_rgba, d_acc, d_mean and d_sd may be nullptr.
int clamp_accumulate_device(const char* at, uint32_t width, uint32_t height, const TemporalParams& prm, const ClampParams& kprm, bool feedback,
                            const double* d_lin, const double* d_normal, const double* d_depth, const double* d_alpha, const double* d_pm1, const double* d_pm2,
                            const double* d_phist, const double* d_plen, const double* d_pnormal, const double* d_pdepth, const double* d_palpha, double* d_m1,
                            uint8_t* d_rgba, double* d_m2, double* d_acc, double* d_len, double* d_xy, double* d_mean, double* d_sd, uint8_t* d_clipped,
                            hipStream_t stream) {
    const dim3 block(CLAMP_BLOCK_X, CLAMP_BLOCK_Y);
    const dim3 grid((width + CLAMP_BLOCK_X - 1) / CLAMP_BLOCK_X, (height + CLAMP_BLOCK_Y - 1) / CLAMP_BLOCK_Y);
    hipLaunchKernelGGL(clamp_accumulate_kernel, grid, block, clamp_lds_bytes(kprm.radius), stream, width, height, prm, kprm, feedback ? 1u : 0u, d_lin, d_normal,
                       d_depth, d_alpha, d_pm1, d_pm2, d_phist, d_plen, d_pnormal, d_pdepth, d_palpha, d_m1, d_rgba, d_m2, d_acc, d_len, d_xy, d_mean, d_sd,
                       d_clipped);
    HIP_TRY_AS(at, hipGetLastError());
    return RTTNW_OK;
}

int clamp_device(uint32_t width, uint32_t height, const TemporalParams& prm, const VarianceParams& vprm, const ClampParams& kprm, const double* linear_rgb,
                 const double* normal, const double* depth, const double* alpha, const double* prev_linear_rgb, const double* prev_moment2_rgb,
                 const double* prev_length, const double* prev_normal, const double* prev_depth, const double* prev_alpha, double* out_linear_rgb,
                 uint8_t* out_rgba8, double* out_moment2_rgb, double* out_length, double* out_prev_xy, double* out_variance_rgb, double* out_mean_rgb,
                 double* out_sd_rgb, uint8_t* out_clipped, double* kernel_ms) {
    FilterCall fc;
    if (int rc = fc.open("temporal_clamp", width, height)) return rc;
    MomentBuffers d;
    DevBuf<double> d_mean, d_sd;
    DevBuf<uint8_t> d_clipped;
    d.stage(fc, prm.has_history != 0, linear_rgb, normal, depth, alpha, prev_linear_rgb, prev_moment2_rgb, prev_length, prev_normal, prev_depth, prev_alpha);
    fc.alloc(d_clipped, 1);
    if (out_mean_rgb) fc.alloc(d_mean, 3);
    if (out_sd_rgb) fc.alloc(d_sd, 3);
    if (int rc = variance_admit_lds(fc.at.c_str(), vprm.radius)) return rc; // stage B's tile; before the clock starts

    if (int rc = fc.start()) return rc;
    if (int rc = clamp_accumulate_device(fc.at.c_str(), width, height, prm, kprm, false, d.lin.p, d.normal.p, d.depth.p, d.alpha.p, d.plin.p, d.pm2.p, nullptr,
                                         d.plen.p, d.pnormal.p, d.pdepth.p, d.palpha.p, d.out.p, d.rgba.p, d.m2.p, nullptr, d.len.p, d.xy.p, d_mean.p, d_sd.p,
                                         d_clipped.p, fc.stream)) return rc;
    if (int rc = variance_passes_device(fc.at.c_str(), width, height, nullptr, vprm, nullptr, d.normal.p, d.depth.p, d.alpha.p, nullptr, nullptr, nullptr, nullptr,
                                        nullptr, nullptr, d.out.p, nullptr, d.m2.p, d.len.p, nullptr, d.var.p, fc.stream)) return rc;
    if (int rc = fc.finish(kernel_ms)) return rc;
    d.copy_out(fc, out_linear_rgb, out_rgba8, out_moment2_rgb, out_length, out_prev_xy, out_variance_rgb);
    fc.copy_out(out_mean_rgb, d_mean, 3);
    fc.copy_out(out_sd_rgb, d_sd, 3);
    fc.copy_out(out_clipped, d_clipped, 1);
    return fc.rc;
}

} // namespace rt
