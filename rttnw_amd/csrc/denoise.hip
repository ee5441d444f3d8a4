// denoise.hip — the device half of rttnw_denoise and rttnw_reconstruct (include/rttnw_hip.h): three small kernels around the per-pixel arithmetic
// of denoise.hpp, one thread per pixel (prepare: per channel value), double throughout (no arithmetic-namespace copies: unfused_mul() keeps the contracted build from fusing anything).
//   atrous_prepare_kernel  demodulate colour and variance by the first-hit albedo
//   atrous_pass_kernel     one à-trous pass at stride 2^i, ping-pong between two colour (and variance) buffers; one launch per pass
//   atrous_finish_kernel   remodulate, write the linear image, its variance and RGBA8
// Each is a template on denoise.hpp's compile-time switch.  Without flags it is rttnw_denoise's kernel, which has no flag argument at all;
// with flags it is rttnw_reconstruct's, which carries the "holds a value" bytes beside the colour — prepare fills the background, the passes
// ping-pong a flag buffer too (a pass never reads a flag it writes), finish writes the out_valid bytes.
// The passes read 25 taps per pixel straight from global memory: the image and its features are a few megabytes, L2-resident, and from the
// third pass on (stride >= 4) the taps of neighbouring pixels no longer share lines a tile in LDS would save.
#include "feature_api.hpp"
#include "filter_call.hpp"
#include "reconstruct.hpp"

namespace rt {
namespace {

// A kernel's flag arguments: pointers with FLAGS, an empty struct without — nothing to load, nothing to pass wrongly
struct NoFlags {};
template <bool FLAGS> using FlagsIn = std::conditional_t<FLAGS, const uint8_t*, NoFlags>;
template <bool FLAGS> using FlagsOut = std::conditional_t<FLAGS, uint8_t*, NoFlags>;
template <bool FLAGS> using PassView = std::conditional_t<FLAGS, ReconstructView, DenoiseView>;

template <bool FLAGS>
__global__ void atrous_prepare_kernel(uint32_t n, const double* __restrict__ colour, const double* __restrict__ variance, const double* __restrict__ albedo,
                                      const double* __restrict__ alpha, double* __restrict__ out_colour, double* __restrict__ out_variance,
                                      FlagsIn<FLAGS> valid, FlagsOut<FLAGS> out_holds) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; // one thread per channel value: a pixel's channels share only its alpha and flag
    if (i >= n * 3u) return;
    const uint32_t pixel = i / 3u;
    bool holds = true;
    if constexpr (FLAGS) holds = valid[pixel] != 0;
    const uint8_t h = atrous_prepare_value<FLAGS>(holds, colour + i, variance ? variance + i : nullptr, albedo[i], alpha[pixel], out_colour + i,
                                                  variance ? out_variance + i : nullptr);
    if constexpr (FLAGS)
        if (i == pixel * 3u) out_holds[pixel] = h;
}

// The pass keeps, argument for argument, the two signatures it had as two kernels — its device code is held to theirs instruction for
// instruction —, so its switch is the pack H: empty without flags, uint8_t with them (the bytes H' the pass writes).
template <typename... H>
__global__ void atrous_pass_kernel(PassView<sizeof...(H) != 0> in, DenoiseParams prm, uint32_t stride, double* __restrict__ out_colour,
                                   double* __restrict__ out_variance, H* __restrict__... out_holds) {
    constexpr bool FLAGS = sizeof...(H) != 0;
    const DenoiseView* img;
    if constexpr (FLAGS) img = &in.img; else img = &in;
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= img->width || y >= img->height) return;
    double c[3], v[3];
    uint8_t holds = 1u;
    if constexpr (FLAGS) holds = reconstruct_filter_pixel(in, prm, x, y, stride, c, v);
    else denoise_filter_pixel(in, prm, x, y, stride, c, v);
    const size_t p = size_t(y) * img->width + x, o = p * 3;
    for (int ch = 0; ch < 3; ++ch) {
        out_colour[o + ch] = c[ch];
        if (img->variance) out_variance[o + ch] = v[ch];
    }
    ((out_holds[p] = holds), ...);
}

template <bool FLAGS>
__global__ void atrous_finish_kernel(uint32_t n, uint32_t remodulate, const double* __restrict__ colour, const double* __restrict__ variance,
                                     const double* __restrict__ albedo, const double* __restrict__ alpha, double* __restrict__ out_colour,
                                     uint8_t* __restrict__ out_rgba8, double* __restrict__ out_variance, FlagsIn<FLAGS> holds, FlagsOut<FLAGS> out_valid) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; // one thread per pixel
    if (i >= n) return;
    const size_t o = size_t(i) * 3;
    bool own = true;
    if constexpr (FLAGS) own = holds[i] != 0;
    const uint8_t ok = atrous_finish_pixel<FLAGS>(own, remodulate != 0u, colour + o, variance ? variance + o : nullptr, albedo + o, alpha[i], out_colour + o,
                                                  out_rgba8 + size_t(i) * 4, variance ? out_variance + o : nullptr);
    if constexpr (FLAGS) out_valid[i] = ok;
}

template <bool FLAGS>
void atrous_enqueue(uint32_t width, uint32_t height, const double* d_in, const double* d_var, const uint8_t* d_valid, const double* d_albedo,
                    const double* d_normal, const double* d_depth, const double* d_alpha, uint32_t iterations, const DenoiseParams& prm,
                    double* const d_c[2], double* const d_v[2], uint8_t* const d_h[2], uint8_t* d_rgba, uint8_t* d_out_valid, hipStream_t stream, int& out,
                    uint32_t tap_after = 0, double* d_tap = nullptr) {
    const auto flags = [](auto* p) { if constexpr (FLAGS) return p; else return NoFlags{}; };
    uint8_t* const no_h[2] = {nullptr, nullptr};
    uint8_t* const* h = FLAGS ? d_h : no_h;
    const uint32_t n = uint32_t(size_t(width) * height);
    const bool has_var = d_var != nullptr;
    const dim3 flat_block(256), value_grid((n * 3u + 255u) / 256u), pixel_grid((n + 255u) / 256u);
    const dim3 block(32, 8), grid((width + 31) / 32, (height + 7) / 8);
    int cur = 0; // d_c[cur] / d_v[cur] / d_h[cur] hold the current image once the first pass has run
    const double *colour = d_in, *variance = d_var;
    const uint8_t* holds = d_valid;
    if (iterations > 0) {
        // iterations == 0 is the identity on the pixels that hold a value: no demodulation, no background fill, the finish step only quantises
        hipLaunchKernelGGL(atrous_prepare_kernel<FLAGS>, value_grid, flat_block, 0, stream, n, d_in, d_var, d_albedo, d_alpha, d_c[0], d_v[0], flags(d_valid),
                           flags(h[0]));
        for (uint32_t i = 0; i < iterations; ++i) {
            const DenoiseView img{width, height, d_c[cur], has_var ? d_v[cur] : nullptr, d_normal, d_depth, d_alpha};
            if constexpr (FLAGS)
                hipLaunchKernelGGL(atrous_pass_kernel<uint8_t>, grid, block, 0, stream, ReconstructView{img, h[cur]}, prm, 1u << i, d_c[cur ^ 1], d_v[cur ^ 1],
                                   h[cur ^ 1]);
            else hipLaunchKernelGGL(atrous_pass_kernel<>, grid, block, 0, stream, img, prm, 1u << i, d_c[cur ^ 1], d_v[cur ^ 1]);
            cur ^= 1;
            // the tap (atrous_passes_tap_device): what the call would return with i + 1 iterations, the finish step's colour alone.  d_rgba is
            // written again by the last finish step, behind this one on the stream.
            if constexpr (!FLAGS)
                if (d_tap && i + 1 == tap_after)
                    hipLaunchKernelGGL(atrous_finish_kernel<false>, pixel_grid, flat_block, 0, stream, n, 1u, d_c[cur], nullptr, d_albedo, d_alpha, d_tap, d_rgba,
                                       nullptr, NoFlags{}, NoFlags{});
        }
        colour = d_c[cur];
        variance = has_var ? d_v[cur] : nullptr;
        holds = h[cur];
    }
    // (the finish step writes into the buffers the last pass read: never the ones it reads itself)
    hipLaunchKernelGGL(atrous_finish_kernel<FLAGS>, pixel_grid, flat_block, 0, stream, n, iterations > 0 ? 1u : 0u, colour, variance, d_albedo, d_alpha,
                       d_c[cur ^ 1], d_rgba, d_v[cur ^ 1], flags(holds), flags(d_out_valid));
    out = cur ^ 1;
}

} // namespace

// The passes on buffers that are already on the device (rttnw_denoise and rttnw_reconstruct behind their uploads; the filtering adaptive forms
// once per round or behind their rounds): prepare, `iterations` passes and the finish step, enqueued on `stream` — nothing else: no allocation,
// no copy, no wait.  d_valid: the "holds a value" bytes, or nullptr where every pixel does (rttnw_denoise's kernels; d_h and d_out_valid are
// then not used).  d_c / d_v / d_h: the two ping-pong buffers of w*h*3 doubles (d_v unused without a variance) and of w*h flag bytes, d_rgba
// w*h*4 bytes, d_out_valid w*h bytes.  `out`: the linear image is left in d_c[out], its variance in d_v[out].
int atrous_passes_device(uint32_t width, uint32_t height, const double* d_in, const double* d_var, const uint8_t* d_valid, const double* d_albedo,
                         const double* d_normal, const double* d_depth, const double* d_alpha, uint32_t iterations, const DenoiseParams& prm,
                         double* const d_c[2], double* const d_v[2], uint8_t* const d_h[2], uint8_t* d_rgba, uint8_t* d_out_valid, hipStream_t stream,
                         int& out) {
    (d_valid ? atrous_enqueue<true> : atrous_enqueue<false>)(width, height, d_in, d_var, d_valid, d_albedo, d_normal, d_depth, d_alpha, iterations, prm, d_c,
                                                              d_v, d_h, d_rgba, d_out_valid, stream, out, 0u, nullptr);
    HIP_TRY_AS(d_valid ? "reconstruct: " : "denoise: ", hipGetLastError());
    return RTTNW_OK;
}

// rttnw_denoise's passes with a TAP of the pass loop (rttnw_svgf_push's feedback): beside everything atrous_passes_device leaves, d_tap (w*h*3)
// receives the linear image the same call would return with `tap_after` iterations, 1 <= tap_after <= iterations — a pass does not depend on how
// many follow it, so this is one more finish step behind pass tap_after, not a second run.  No flags: every pixel holds a value.
int atrous_passes_tap_device(uint32_t width, uint32_t height, const double* d_in, const double* d_var, const double* d_albedo, const double* d_normal,
                             const double* d_depth, const double* d_alpha, uint32_t iterations, const DenoiseParams& prm, double* const d_c[2],
                             double* const d_v[2], uint8_t* d_rgba, uint32_t tap_after, double* d_tap, hipStream_t stream, int& out) {
    atrous_enqueue<false>(width, height, d_in, d_var, nullptr, d_albedo, d_normal, d_depth, d_alpha, iterations, prm, d_c, d_v, nullptr, d_rgba, nullptr,
                          stream, out, tap_after, d_tap);
    HIP_TRY_AS("svgf: ", hipGetLastError());
    return RTTNW_OK;
}

// rttnw_denoise's (`call` "denoise", valid == nullptr) and rttnw_reconstruct's ("reconstruct") device half: the caller's arrays and the
// workspace on the device, the passes between two events, the outputs the caller asked for.
int atrous_device(const char* call, uint32_t width, uint32_t height, const double* linear_rgb, const double* variance_rgb, const uint8_t* valid,
                  const double* albedo, const double* normal, const double* depth, const double* alpha, uint32_t iterations, const DenoiseParams& prm,
                  double* out_linear_rgb, uint8_t* out_rgba8, double* out_variance_rgb, uint8_t* out_valid, double* kernel_ms) {
    FilterCall fc;
    if (int rc = fc.open(call, width, height)) return rc;
    const bool has_var = variance_rgb != nullptr, has_flags = valid != nullptr;
    DevBuf<double> d_in, d_var, d_albedo, d_normal, d_depth, d_alpha, d_c[2], d_v[2];
    DevBuf<uint8_t> d_valid, d_h[2], d_rgba, d_out_valid;
    fc.upload(d_in, linear_rgb, 3);
    if (has_var) fc.upload(d_var, variance_rgb, 3);
    fc.upload(d_albedo, albedo, 3);
    fc.upload(d_normal, normal, 3);
    fc.upload(d_depth, depth, 1);
    fc.upload(d_alpha, alpha, 1);
    if (has_flags) fc.upload(d_valid, valid, 1);
    for (int k = 0; k < 2; ++k) {
        fc.alloc(d_c[k], 3);
        if (has_var) fc.alloc(d_v[k], 3);
        if (has_flags) fc.alloc(d_h[k], 1);
    }
    fc.alloc(d_rgba, 4);
    if (has_flags) fc.alloc(d_out_valid, 1);

    // the passes step, between the two events
    double* const c[2] = {d_c[0].p, d_c[1].p};
    double* const v[2] = {d_v[0].p, d_v[1].p};
    uint8_t* const h[2] = {d_h[0].p, d_h[1].p};
    int out = 0;
    if (int rc = fc.start()) return rc;
    if (int rc = atrous_passes_device(width, height, d_in.p, has_var ? d_var.p : nullptr, d_valid.p, d_albedo.p, d_normal.p, d_depth.p, d_alpha.p, iterations,
                                      prm, c, v, h, d_rgba.p, d_out_valid.p, fc.stream, out)) return rc;
    if (int rc = fc.finish(kernel_ms)) return rc;
    fc.copy_out(out_linear_rgb, c[out], 3);
    fc.copy_out(out_rgba8, d_rgba, 4);
    if (has_var) fc.copy_out(out_variance_rgb, v[out], 3);
    if (has_flags) fc.copy_out(out_valid, d_out_valid, 1);
    return fc.rc;
}

} // namespace rt
