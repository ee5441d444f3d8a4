// denoise.hip — the device half of rttnw_denoise (include/rttnw_hip.h): three small kernels around the per-pixel arithmetic of denoise.hpp,
// one thread per pixel, double throughout (no arithmetic-namespace copies: unfused_mul() keeps the contracted build from fusing anything).
//   denoise_prepare_kernel  demodulate colour and variance by the first-hit albedo
//   denoise_pass_kernel     one à-trous pass at stride 2^i, ping-pong between two colour (and variance) buffers; one launch per pass
//   denoise_finish_kernel   remodulate, write the linear image, its variance and RGBA8
// The passes read 25 taps per pixel straight from global memory: the image and its features are a few megabytes, L2-resident, and from the
// third pass on (stride >= 4) the taps of neighbouring pixels no longer share lines a tile in LDS would save.
#include "feature_api.hpp"

namespace rt {
namespace {

__global__ void denoise_prepare_kernel(uint32_t n, const double* __restrict__ colour, const double* __restrict__ variance, const double* __restrict__ albedo,
                                       const double* __restrict__ alpha, double* __restrict__ out_colour, double* __restrict__ out_variance) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; // one thread per channel value
    if (i >= n * 3u) return;
    const double a = alpha[i / 3u];
    out_colour[i] = denoise_demodulate(colour[i], albedo[i], a);
    if (variance) out_variance[i] = denoise_demodulate_variance(variance[i], albedo[i], a);
}

__global__ void denoise_pass_kernel(DenoiseView in, DenoiseParams prm, uint32_t stride, double* __restrict__ out_colour, double* __restrict__ out_variance) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= in.width || y >= in.height) return;
    double c[3], v[3];
    denoise_filter_pixel(in, prm, x, y, stride, c, v);
    const size_t o = (size_t(y) * in.width + x) * 3;
    for (int ch = 0; ch < 3; ++ch) {
        out_colour[o + ch] = c[ch];
        if (in.variance) out_variance[o + ch] = v[ch];
    }
}

__global__ void denoise_finish_kernel(uint32_t n, uint32_t remodulate, const double* __restrict__ colour, const double* __restrict__ variance,
                                      const double* __restrict__ albedo, const double* __restrict__ alpha, double* __restrict__ out_colour,
                                      uint8_t* __restrict__ out_rgba8, double* __restrict__ out_variance) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; // one thread per pixel
    if (i >= n) return;
    for (uint32_t ch = 0; ch < 3u; ++ch) {
        const uint32_t k = i * 3u + ch;
        const double c = remodulate ? denoise_remodulate(colour[k], albedo[k], alpha[i]) : colour[k];
        out_colour[k] = c;
        out_rgba8[i * 4u + ch] = denoise_quantise(c);
        if (variance) out_variance[k] = remodulate ? denoise_remodulate_variance(variance[k], albedo[k], alpha[i]) : variance[k];
    }
    out_rgba8[i * 4u + 3u] = 255;
}

} // namespace

#define DENOISE_TRY(expr)                                                                              \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            set_last_error(std::string("denoise: " #expr ": ") + hipGetErrorString(e_));              \
            return RTTNW_ERR_HIP;                                                                      \
        }                                                                                              \
    } while (0)

// The passes on buffers that are already on the device (rttnw_denoise behind its uploads; rttnw_render_adaptive_denoised once per round):
// prepare, `iterations` passes and the finish step, enqueued on `stream` — nothing else: no allocation, no copy, no wait.  d_c / d_v: the two
// ping-pong buffers of w*h*3 doubles each (d_v unused without a variance), d_rgba w*h*4 bytes.  `out`: the linear image is left in d_c[out],
// its variance in d_v[out].
int denoise_passes_device(uint32_t width, uint32_t height, const double* d_in, const double* d_var, const double* d_albedo, const double* d_normal,
                          const double* d_depth, const double* d_alpha, uint32_t iterations, const DenoiseParams& prm, double* const d_c[2],
                          double* const d_v[2], uint8_t* d_rgba, hipStream_t stream, int& out) {
    const uint32_t n = uint32_t(size_t(width) * height);
    const bool has_var = d_var != nullptr;
    const dim3 flat_block(256), value_grid((n * 3u + 255u) / 256u), pixel_grid((n + 255u) / 256u);
    const dim3 block(32, 8), grid((width + 31) / 32, (height + 7) / 8);
    int cur = 0; // d_c[cur] / d_v[cur] hold the current image once the first pass has run
    const double *colour = d_in, *variance = d_var;
    if (iterations > 0) {
        // iterations == 0 is the identity: no demodulation either, the finish step only quantises
        hipLaunchKernelGGL(denoise_prepare_kernel, value_grid, flat_block, 0, stream, n, d_in, variance, d_albedo, d_alpha, d_c[0], d_v[0]);
        for (uint32_t i = 0; i < iterations; ++i) {
            DenoiseView view{width, height, d_c[cur], has_var ? d_v[cur] : nullptr, d_normal, d_depth, d_alpha};
            hipLaunchKernelGGL(denoise_pass_kernel, grid, block, 0, stream, view, prm, 1u << i, d_c[cur ^ 1], d_v[cur ^ 1]);
            cur ^= 1;
        }
        colour = d_c[cur];
        variance = has_var ? d_v[cur] : nullptr;
    }
    // (the finish step writes into the buffers the last pass read: never the ones it reads itself)
    hipLaunchKernelGGL(denoise_finish_kernel, pixel_grid, flat_block, 0, stream, n, iterations > 0 ? 1u : 0u, colour, variance, d_albedo, d_alpha,
                       d_c[cur ^ 1], d_rgba, d_v[cur ^ 1]);
    DENOISE_TRY(hipGetLastError());
    out = cur ^ 1;
    return RTTNW_OK;
}

int denoise_device(uint32_t width, uint32_t height, const double* linear_rgb, const double* variance_rgb, const double* albedo, const double* normal,
                   const double* depth, const double* alpha, uint32_t iterations, const DenoiseParams& prm, double* out_linear_rgb, uint8_t* out_rgba8,
                   double* out_variance_rgb, double* kernel_ms) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        set_last_error("denoise: no HIP device available (this library has no CPU fallback)");
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
    DevBuf<uint8_t> d_rgba;
    DENOISE_TRY(upload(d_in, linear_rgb, npx * 3));
    if (has_var) DENOISE_TRY(upload(d_var, variance_rgb, npx * 3));
    DENOISE_TRY(upload(d_albedo, albedo, npx * 3));
    DENOISE_TRY(upload(d_normal, normal, npx * 3));
    DENOISE_TRY(upload(d_depth, depth, npx));
    DENOISE_TRY(upload(d_alpha, alpha, npx));
    for (int k = 0; k < 2; ++k) {
        DENOISE_TRY(d_c[k].alloc(npx * 3));
        if (has_var) DENOISE_TRY(d_v[k].alloc(npx * 3));
    }
    DENOISE_TRY(d_rgba.alloc(npx * 4));
    Event ev0, ev1;
    DENOISE_TRY(create_event(ev0));
    DENOISE_TRY(create_event(ev1));

    // the passes step, between the two events
    const hipStream_t stream = nullptr;
    double* const c[2] = {d_c[0].p, d_c[1].p};
    double* const v[2] = {d_v[0].p, d_v[1].p};
    int out = 0;
    DENOISE_TRY(hipEventRecord(ev0.get(), stream));
    if (int rc = denoise_passes_device(width, height, d_in.p, has_var ? d_var.p : nullptr, d_albedo.p, d_normal.p, d_depth.p, d_alpha.p, iterations, prm, c, v,
                                       d_rgba.p, stream, out)) return rc;
    DENOISE_TRY(hipEventRecord(ev1.get(), stream));
    DENOISE_TRY(hipDeviceSynchronize());
    if (kernel_ms) {
        float ms = 0;
        DENOISE_TRY(hipEventElapsedTime(&ms, ev0.get(), ev1.get()));
        *kernel_ms = ms;
    }
    if (out_linear_rgb) DENOISE_TRY(hipMemcpy(out_linear_rgb, c[out], npx * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (out_rgba8) DENOISE_TRY(hipMemcpy(out_rgba8, d_rgba.p, npx * 4, hipMemcpyDeviceToHost));
    if (out_variance_rgb && has_var) DENOISE_TRY(hipMemcpy(out_variance_rgb, v[out], npx * 3 * sizeof(double), hipMemcpyDeviceToHost));
    return RTTNW_OK;
}

} // namespace rt
