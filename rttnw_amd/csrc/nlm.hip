// nlm.hip — the device half of rttnw_denoise_nlm (include/rttnw_hip.h) around the arithmetic of nlm.hpp, double throughout:
//   nlm_variance_kernel  the pair variance (only when the caller gave none), one thread per channel value
//   nlm_filter_kernel    one block per TxT tile and direction (blockIdx.z 0: guide B weighs half A; 1: guide A weighs half B), one thread per pixel
//   nlm_finish_kernel    the mean of the two filtered halves, its RGBA8 and the error estimate
// The filter kernel stages the tile's guide and variance, with a halo of r + f, in LDS as six planes (r, g, b of each: consecutive lanes read
// consecutive doubles, which ds_read_b64 serves without a bank conflict), then walks the (2r+1)^2 offsets row-major.  Per offset: every
// delta(x, o) of the tile and its patch halo is formed ONCE into LDS ((T + 2f)^2 of them: three f64 divisions each — what bounds the kernel),
// the row sums of the patches are built from those, and each pixel's thread adds 2f + 1 row sums, turns them into its weight and accumulates
// the candidate of the other half, which it reads from global memory (a 3-double read per offset and pixel, L1/L2-resident).  Two barriers
// per offset.  T = 32 where its LDS fits a CU (148 KiB at the default radii: one block of 16 waves per CU; 1.4 deltas per pixel and offset),
// T = 16 otherwise (155 KiB at r 16, f 4; 1.9 and more deltas per pixel and offset).  DESIGN.md §10b has the measured times.
#include "feature_api.hpp"
#include "filter_call.hpp"
#include "nlm.hpp"

namespace rt {
namespace {


__global__ void nlm_variance_kernel(uint32_t width, uint32_t height, const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; // one thread per channel value
    if (i >= width * height * 3u) return;
    const uint32_t pixel = i / 3u;
    out[i] = nlm_pair_variance(width, height, a, b, pixel % width, pixel / width, int(i - pixel * 3u));
}

template <int T> // the tile's side; one thread per pixel of the tile
__global__ __launch_bounds__(T * T) void nlm_filter_kernel(NlmView in, NlmParams prm, double* __restrict__ out_a, double* __restrict__ out_b) {
    extern __shared__ __attribute__((aligned(16))) double nlm_lds[];
    constexpr int NLM_BLOCK = T * T;
    const int r = int(prm.r), f = int(prm.f), halo = r + f;
    const int E = T + 2 * halo, P = T + 2 * f, plane = E * E; // the staged region's side, the delta region's side
    double* G = nlm_lds;                                       // [3][E][E] the guide
    double* V = nlm_lds + 3 * plane;                           // [3][E][E] its variance
    double* Dl = nlm_lds + 6 * plane;                          // [P][P] delta(x, o) of the current offset
    double* Rl = Dl + P * P;                                   // [P][T] the row sums
    const bool second = blockIdx.z != 0;
    const double* __restrict__ guide = second ? in.a : in.b;
    const double* __restrict__ var = second ? in.var_a : in.var_b;
    const double* __restrict__ src = second ? in.b : in.a;
    const int x0 = int(blockIdx.x) * T, y0 = int(blockIdx.y) * T;
    const int tid = int(threadIdx.x);

    for (int i = tid; i < plane; i += NLM_BLOCK) {
        const int ey = i / E, ex = i - ey * E;
        const size_t q = (size_t(nlm_clamp(y0 - halo, ey, in.height)) * in.width + nlm_clamp(x0 - halo, ex, in.width)) * 3;
        for (int ch = 0; ch < 3; ++ch) {
            G[ch * plane + i] = guide[q + ch];
            V[ch * plane + i] = var[q + ch];
        }
    }
    __syncthreads();

    const int px = tid % T, py = tid / T;
    double sum_w = 0.0, sum_c[3] = {0.0, 0.0, 0.0};
    for (int oy = -r; oy <= r; ++oy)
        for (int ox = -r; ox <= r; ++ox) {
            double w = 1.0; // the centre offset
            if (ox != 0 || oy != 0) { // (uniform over the block: the barriers below are reached by all of its threads or by none)
                for (int i = tid; i < P * P; i += NLM_BLOCK) {
                    const int dy = i / P, dx = i - dy * P;
                    const int xs = (dy + r) * E + dx + r, qs = xs + oy * E + ox; // 0 <= dy + r + oy, dx + r + ox < E
                    const double d0 = nlm_delta_channel(G[xs], G[qs], V[xs], V[qs], prm.k2);
                    const double d1 = nlm_delta_channel(G[plane + xs], G[plane + qs], V[plane + xs], V[plane + qs], prm.k2);
                    const double d2 = nlm_delta_channel(G[2 * plane + xs], G[2 * plane + qs], V[2 * plane + xs], V[2 * plane + qs], prm.k2);
                    Dl[i] = nlm_delta(d0, d1, d2);
                }
                __syncthreads();
                for (int i = tid; i < P * T; i += NLM_BLOCK) {
                    const int ry = i / T, rx = i - ry * T;
                    double sum = 0.0;
                    for (int n = 0; n <= 2 * f; ++n) sum = sum + Dl[ry * P + rx + n];
                    Rl[i] = sum;
                }
                __syncthreads();
                double column = 0.0;
                for (int n = 0; n <= 2 * f; ++n) column = column + Rl[(py + n) * T + px];
                w = nlm_weight(column, prm.patch_taps);
            }
            const size_t q = (size_t(nlm_clamp(y0 + py, oy, in.height)) * in.width + nlm_clamp(x0 + px, ox, in.width)) * 3;
            sum_w = sum_w + w;
            for (int ch = 0; ch < 3; ++ch) sum_c[ch] = sum_c[ch] + unfused_mul(w, src[q + ch]);
        }
    const uint32_t x = uint32_t(x0 + px), y = uint32_t(y0 + py);
    if (x >= in.width || y >= in.height) return;
    double* dst = (second ? out_b : out_a) + (size_t(y) * in.width + x) * 3;
    for (int ch = 0; ch < 3; ++ch) dst[ch] = sum_c[ch] / sum_w;
}

__global__ void nlm_finish_kernel(uint32_t n, const double* __restrict__ fa, const double* __restrict__ fb, double* __restrict__ out,
                                  uint8_t* __restrict__ out_rgba8, double* __restrict__ out_error) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; // one thread per channel value
    if (i >= n * 3u) return;
    const uint32_t pixel = i / 3u, ch = i - pixel * 3u;
    const double c = nlm_mean(fa[i], fb[i]);
    out[i] = c;
    out_error[i] = nlm_error(fa[i], fb[i]);
    out_rgba8[pixel * 4u + ch] = denoise_quantise(c);
    if (ch == 0u) out_rgba8[pixel * 4u + 3u] = 255;
}

} // namespace

// The filter kernel a call's radii take, with its dynamic LDS admitted: what a caller settles before it starts its clock.
int nlm_plan_device(const char* at, const NlmParams& prm, NlmPlan& plan) {
    // the large tile where its LDS fits a CU, the small one — which fits at every radius the entry point accepts — otherwise
    const bool large = nlm_lds_bytes(NLM_TILE_LARGE, prm.r, prm.f) <= NLM_LDS_BYTES;
    plan.tile = large ? NLM_TILE_LARGE : NLM_TILE_SMALL;
    plan.lds_bytes = nlm_lds_bytes(plan.tile, prm.r, prm.f);
    plan.filter = large ? nlm_filter_kernel<int(NLM_TILE_LARGE)> : nlm_filter_kernel<int(NLM_TILE_SMALL)>;
    HIP_TRY_AS(at, hipFuncSetAttribute(reinterpret_cast<const void*>(plan.filter), hipFuncAttributeMaxDynamicSharedMemorySize, int(plan.lds_bytes)));
    return RTTNW_OK;
}

// The filter's kernels on buffers that are already on the device (rttnw_denoise_nlm behind its uploads; rttnw_denoise_select between its à-trous
// runs and its selection), enqueued on `stream` — nothing else: no allocation, no copy, no wait.  d_var_a / d_var_b: the guides' variances, or
// both nullptr: the pair variance is then formed into d_pair_var (w*h*3), which serves both guides.  d_fa / d_fb (w*h*3 each) take the two
// cross-filtered halves.  d_out, d_err (w*h*3) and d_rgba (w*h*4) take the mean, the error estimate and the RGBA8 — or d_out == nullptr: the
// finish step is not run and the other two are not used.
int nlm_passes_device(const char* at, uint32_t width, uint32_t height, const double* d_a, const double* d_b, const double* d_var_a, const double* d_var_b,
                      double* d_pair_var, const NlmParams& prm, const NlmPlan& plan, double* d_fa, double* d_fb, double* d_out, uint8_t* d_rgba,
                      double* d_err, hipStream_t stream) {
    const size_t npx = size_t(width) * height;
    const bool has_var = d_var_a != nullptr;
    const dim3 flat_block(256), value_grid(uint32_t((npx * 3 + 255) / 256));
    const dim3 tiles((width + plan.tile - 1) / plan.tile, (height + plan.tile - 1) / plan.tile, 2);
    if (!has_var) hipLaunchKernelGGL(nlm_variance_kernel, value_grid, flat_block, 0, stream, width, height, d_a, d_b, d_pair_var);
    const NlmView view{width, height, d_a, d_b, has_var ? d_var_a : d_pair_var, has_var ? d_var_b : d_pair_var};
    hipLaunchKernelGGL(plan.filter, tiles, dim3(plan.tile * plan.tile), plan.lds_bytes, stream, view, prm, d_fa, d_fb);
    if (d_out) hipLaunchKernelGGL(nlm_finish_kernel, value_grid, flat_block, 0, stream, uint32_t(npx), d_fa, d_fb, d_out, d_rgba, d_err);
    HIP_TRY_AS(at, hipGetLastError());
    return RTTNW_OK;
}

// rttnw_denoise_nlm's device half: the caller's arrays and the workspace on the device, the kernels between two events, the outputs the
// caller asked for.
int nlm_device(uint32_t width, uint32_t height, const double* half_a, const double* half_b, const double* var_a, const double* var_b, const NlmParams& prm,
               double* out_linear_rgb, uint8_t* out_rgba8, double* out_half_a, double* out_half_b, double* out_error_rgb, double* kernel_ms) {
    FilterCall fc;
    if (int rc = fc.open("denoise_nlm", width, height)) return rc;
    const bool has_var = var_a != nullptr;
    DevBuf<double> d_a, d_b, d_va, d_vb, d_fa, d_fb, d_out, d_err;
    DevBuf<uint8_t> d_rgba;
    fc.upload(d_a, half_a, 3);
    fc.upload(d_b, half_b, 3);
    if (has_var) {
        fc.upload(d_va, var_a, 3);
        fc.upload(d_vb, var_b, 3);
    } else {
        fc.alloc(d_va, 3); // the pair variance: one array for both guides
    }
    fc.alloc(d_fa, 3);
    fc.alloc(d_fb, 3);
    fc.alloc(d_out, 3);
    fc.alloc(d_err, 3);
    fc.alloc(d_rgba, 4);
    NlmPlan plan;
    if (int rc = nlm_plan_device(fc.at.c_str(), prm, plan)) return rc; // before the clock starts

    if (int rc = fc.start()) return rc;
    if (int rc = nlm_passes_device(fc.at.c_str(), width, height, d_a.p, d_b.p, has_var ? d_va.p : nullptr, has_var ? d_vb.p : nullptr, has_var ? nullptr : d_va.p,
                                   prm, plan, d_fa.p, d_fb.p, d_out.p, d_rgba.p, d_err.p, fc.stream)) return rc;
    if (int rc = fc.finish(kernel_ms)) return rc;
    fc.copy_out(out_linear_rgb, d_out, 3);
    fc.copy_out(out_rgba8, d_rgba, 4);
    fc.copy_out(out_half_a, d_fa, 3);
    fc.copy_out(out_half_b, d_fb, 3);
    fc.copy_out(out_error_rgb, d_err, 3);
    return fc.rc;
}

} // namespace rt
