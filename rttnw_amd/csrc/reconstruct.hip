// reconstruct.hip — the device half of rttnw_reconstruct (include/rttnw_hip.h): denoise.hip's three kernels with the "holds a value" flag of
// reconstruct.hpp carried beside the colour, one thread per pixel, double throughout.
//   reconstruct_prepare_kernel  demodulate the pixels that hold a value; a pixel without one whose alpha is 0 takes the background
//   reconstruct_pass_kernel     one à-trous pass at stride 2^i, ping-pong between two colour, variance AND flag buffers: a pass never reads a flag it writes
//   reconstruct_finish_kernel   remodulate, write the linear image, its variance, RGBA8 and the out_valid bytes
// No LDS tile, for denoise.hip's reason: the image and its features are L2-resident, and from stride 4 on neighbouring pixels share no lines.
// The alive-byte and valid-byte kernels of rttnw_render_preview (render_api.cpp) live here too: they only read and write bytes and counts.
#include "feature_api.hpp"
#include "reconstruct.hpp"
#include "rt_core.hpp"

namespace rt {
namespace {

__global__ void reconstruct_prepare_kernel(uint32_t n, const double* __restrict__ colour, const double* __restrict__ variance, const uint8_t* __restrict__ valid,
                                           const double* __restrict__ albedo, const double* __restrict__ alpha, double* __restrict__ out_colour,
                                           double* __restrict__ out_variance, uint8_t* __restrict__ out_holds) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; // one thread per pixel
    if (i >= n) return;
    const size_t o = size_t(i) * 3;
    out_holds[i] = reconstruct_prepare_pixel(valid[i] != 0, colour + o, variance ? variance + o : nullptr, albedo + o, alpha[i], out_colour + o,
                                             variance ? out_variance + o : nullptr);
}

__global__ void reconstruct_pass_kernel(ReconstructView in, DenoiseParams prm, uint32_t stride, double* __restrict__ out_colour,
                                        double* __restrict__ out_variance, uint8_t* __restrict__ out_holds) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= in.img.width || y >= in.img.height) return;
    double c[3], v[3];
    const uint8_t holds = reconstruct_filter_pixel(in, prm, x, y, stride, c, v);
    const size_t p = size_t(y) * in.img.width + x, o = p * 3;
    for (int ch = 0; ch < 3; ++ch) {
        out_colour[o + ch] = c[ch];
        if (in.img.variance) out_variance[o + ch] = v[ch];
    }
    out_holds[p] = holds;
}

__global__ void reconstruct_finish_kernel(uint32_t n, uint32_t remodulate, const double* __restrict__ colour, const double* __restrict__ variance,
                                          const uint8_t* __restrict__ holds, const double* __restrict__ albedo, const double* __restrict__ alpha,
                                          double* __restrict__ out_colour, uint8_t* __restrict__ out_rgba8, double* __restrict__ out_variance,
                                          uint8_t* __restrict__ out_valid) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; // one thread per pixel
    if (i >= n) return;
    const size_t o = size_t(i) * 3;
    out_valid[i] = reconstruct_finish_pixel(holds[i] != 0, remodulate != 0u, colour + o, variance ? variance + o : nullptr, albedo + o, alpha[i],
                                            out_colour + o, out_rgba8 + size_t(i) * 4, variance ? out_variance + o : nullptr);
}

// rttnw_render_preview, before round 0: the alive byte of every packed pixel of a frame that lives on one rank — 1 on the lattice
// x % 2^level == 0 && y % 2^level == 0, 0 elsewhere (the buffer was cleared: the rest of an edge tile stays 0)
__global__ void preview_lattice_kernel(uint8_t* __restrict__ alive, uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t level) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= width || y >= height) return;
    const uint32_t low = (1u << level) - 1u;
    alive[tile_permuted(x >> 3, y >> 3, tiles_x) * 64ull + ((y & 7u) << 3) + (x & 7u)] = ((x | y) & low) == 0u ? 1u : 0u;
}

// ... and behind the rounds: a pixel holds a value where it holds samples
__global__ void preview_valid_kernel(uint32_t n, const uint32_t* __restrict__ spp, uint8_t* __restrict__ valid) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) valid[i] = spp[i] != 0u ? 1u : 0u;
}

} // namespace

#define RECONSTRUCT_TRY(expr)                                                                          \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            set_last_error(std::string("reconstruct: " #expr ": ") + hipGetErrorString(e_));          \
            return RTTNW_ERR_HIP;                                                                      \
        }                                                                                              \
    } while (0)

// The passes on buffers that are already on the device (rttnw_reconstruct behind its uploads; rttnw_render_preview behind its rounds): prepare,
// `iterations` passes and the finish step, enqueued on `stream` — nothing else: no allocation, no copy, no wait.  d_c / d_v / d_h: the two
// ping-pong buffers of w*h*3 doubles (d_v unused without a variance) and of w*h flag bytes, d_rgba w*h*4 bytes, d_out_valid w*h bytes.
// `out`: the linear image is left in d_c[out], its variance in d_v[out].
int reconstruct_passes_device(uint32_t width, uint32_t height, const double* d_in, const double* d_var, const uint8_t* d_valid, const double* d_albedo,
                              const double* d_normal, const double* d_depth, const double* d_alpha, uint32_t iterations, const DenoiseParams& prm,
                              double* const d_c[2], double* const d_v[2], uint8_t* const d_h[2], uint8_t* d_rgba, uint8_t* d_out_valid,
                              hipStream_t stream, int& out) {
    const uint32_t n = uint32_t(size_t(width) * height);
    const bool has_var = d_var != nullptr;
    const dim3 flat_block(256), pixel_grid((n + 255u) / 256u);
    const dim3 block(32, 8), grid((width + 31) / 32, (height + 7) / 8);
    int cur = 0; // d_c[cur] / d_v[cur] / d_h[cur] hold the current image once the first pass has run
    const double *colour = d_in, *variance = d_var;
    const uint8_t* holds = d_valid;
    if (iterations > 0) {
        // iterations == 0 copies the pixels that hold a value: no demodulation, no background fill, the finish step only quantises
        hipLaunchKernelGGL(reconstruct_prepare_kernel, pixel_grid, flat_block, 0, stream, n, d_in, d_var, d_valid, d_albedo, d_alpha, d_c[0], d_v[0],
                           d_h[0]);
        for (uint32_t i = 0; i < iterations; ++i) {
            ReconstructView view{{width, height, d_c[cur], has_var ? d_v[cur] : nullptr, d_normal, d_depth, d_alpha}, d_h[cur]};
            hipLaunchKernelGGL(reconstruct_pass_kernel, grid, block, 0, stream, view, prm, 1u << i, d_c[cur ^ 1], d_v[cur ^ 1], d_h[cur ^ 1]);
            cur ^= 1;
        }
        colour = d_c[cur];
        variance = has_var ? d_v[cur] : nullptr;
        holds = d_h[cur];
    }
    // (the finish step writes into the buffers the last pass read: never the ones it reads itself)
    hipLaunchKernelGGL(reconstruct_finish_kernel, pixel_grid, flat_block, 0, stream, n, iterations > 0 ? 1u : 0u, colour, variance, holds, d_albedo,
                       d_alpha, d_c[cur ^ 1], d_rgba, d_v[cur ^ 1], d_out_valid);
    RECONSTRUCT_TRY(hipGetLastError());
    out = cur ^ 1;
    return RTTNW_OK;
}

int reconstruct_device(uint32_t width, uint32_t height, const double* linear_rgb, const double* variance_rgb, const uint8_t* valid, const double* albedo,
                       const double* normal, const double* depth, const double* alpha, uint32_t iterations, const DenoiseParams& prm,
                       double* out_linear_rgb, uint8_t* out_rgba8, double* out_variance_rgb, uint8_t* out_valid, double* kernel_ms) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        set_last_error("reconstruct: no HIP device available (this library has no CPU fallback)");
        return RTTNW_ERR_HIP;
    }
    const size_t npx = size_t(width) * height;
    const bool has_var = variance_rgb != nullptr;
    // the upload step: the caller's arrays and the workspace on the device
    auto upload = [](DevBuf<double>& b, const double* src, size_t count) -> hipError_t {
        hipError_t e = b.alloc(count);
        if (e == hipSuccess) e = hipMemcpy(b.p, src, count * sizeof(double), hipMemcpyHostToDevice);
        return e;
    };
    DevBuf<double> d_in, d_var, d_albedo, d_normal, d_depth, d_alpha, d_c[2], d_v[2];
    DevBuf<uint8_t> d_valid, d_h[2], d_rgba, d_out_valid;
    RECONSTRUCT_TRY(upload(d_in, linear_rgb, npx * 3));
    if (has_var) RECONSTRUCT_TRY(upload(d_var, variance_rgb, npx * 3));
    RECONSTRUCT_TRY(upload(d_albedo, albedo, npx * 3));
    RECONSTRUCT_TRY(upload(d_normal, normal, npx * 3));
    RECONSTRUCT_TRY(upload(d_depth, depth, npx));
    RECONSTRUCT_TRY(upload(d_alpha, alpha, npx));
    RECONSTRUCT_TRY(d_valid.alloc(npx));
    RECONSTRUCT_TRY(hipMemcpy(d_valid.p, valid, npx, hipMemcpyHostToDevice));
    for (int k = 0; k < 2; ++k) {
        RECONSTRUCT_TRY(d_c[k].alloc(npx * 3));
        if (has_var) RECONSTRUCT_TRY(d_v[k].alloc(npx * 3));
        RECONSTRUCT_TRY(d_h[k].alloc(npx));
    }
    RECONSTRUCT_TRY(d_rgba.alloc(npx * 4));
    RECONSTRUCT_TRY(d_out_valid.alloc(npx));
    Event ev0, ev1;
    RECONSTRUCT_TRY(create_event(ev0));
    RECONSTRUCT_TRY(create_event(ev1));

    // the passes step, between the two events
    const hipStream_t stream = nullptr;
    double* const c[2] = {d_c[0].p, d_c[1].p};
    double* const v[2] = {d_v[0].p, d_v[1].p};
    uint8_t* const h[2] = {d_h[0].p, d_h[1].p};
    int out = 0;
    RECONSTRUCT_TRY(hipEventRecord(ev0.get(), stream));
    if (int rc = reconstruct_passes_device(width, height, d_in.p, has_var ? d_var.p : nullptr, d_valid.p, d_albedo.p, d_normal.p, d_depth.p, d_alpha.p,
                                           iterations, prm, c, v, h, d_rgba.p, d_out_valid.p, stream, out)) return rc;
    RECONSTRUCT_TRY(hipEventRecord(ev1.get(), stream));
    RECONSTRUCT_TRY(hipDeviceSynchronize());
    if (kernel_ms) {
        float ms = 0;
        RECONSTRUCT_TRY(hipEventElapsedTime(&ms, ev0.get(), ev1.get()));
        *kernel_ms = ms;
    }
    if (out_linear_rgb) RECONSTRUCT_TRY(hipMemcpy(out_linear_rgb, c[out], npx * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (out_rgba8) RECONSTRUCT_TRY(hipMemcpy(out_rgba8, d_rgba.p, npx * 4, hipMemcpyDeviceToHost));
    if (out_variance_rgb && has_var) RECONSTRUCT_TRY(hipMemcpy(out_variance_rgb, v[out], npx * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (out_valid) RECONSTRUCT_TRY(hipMemcpy(out_valid, d_out_valid.p, npx, hipMemcpyDeviceToHost));
    return RTTNW_OK;
}

// rttnw_render_preview's two byte kernels, enqueued on `stream`
int preview_lattice_launch(uint8_t* d_alive, uint32_t pixels_per_rank, uint32_t width, uint32_t height, uint32_t level, hipStream_t stream) {
    rttnw_tile_layout L;
    fill_layout(width, height, 1, L);
    RECONSTRUCT_TRY(hipMemsetAsync(d_alive, 0, pixels_per_rank, stream));
    hipLaunchKernelGGL(preview_lattice_kernel, dim3((width + 31) / 32, (height + 7) / 8), dim3(32, 8), 0, stream, d_alive, width, height, L.tiles_x, level);
    RECONSTRUCT_TRY(hipGetLastError());
    return RTTNW_OK;
}
int preview_valid_launch(const uint32_t* d_spp, uint8_t* d_valid, uint32_t width, uint32_t height, hipStream_t stream) {
    const uint32_t n = uint32_t(size_t(width) * height);
    hipLaunchKernelGGL(preview_valid_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, n, d_spp, d_valid);
    RECONSTRUCT_TRY(hipGetLastError());
    return RTTNW_OK;
}

} // namespace rt
