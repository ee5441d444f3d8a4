// select.hip — the device half of rttnw_denoise_select (include/rttnw_hip.h) around the arithmetic of select.hpp, double throughout.  The halves,
// their variances and the features are uploaded once; the à-trous passes (denoise.hip atrous_passes_device) run twice over them, once per half,
// sharing the feature buffers; the non-local-means kernels (nlm.hip nlm_passes_device) run on the same buffers; then the selection:
//   select_difference_kernel  d of every pixel from the four filtered halves and the two raw ones, one thread per pixel
//   select_blend_kernel       one block per 32x32 tile, one thread per pixel: window sums, choice, blend weight, blend, RGBA8 and error
// The blend kernel keeps everything between d and the output in LDS: d is staged with a halo of s + t (consecutive lanes on consecutive
// doubles, which ds_read_b64 serves without a bank conflict), its row sums are taken over the tile and a halo of t in x, their column sums give
// m on the tile and a halo of t, m's row sums and their column sums give beta.  A position of m's halo that lies outside the image is not the
// window sum around that position but m of the nearest pixel inside (the contract clamps the coordinate of m, then the window's): that pixel
// lies inside the block's own m region, so the second stage reads m through clamped indices.  Four barriers per tile.
#include "feature_api.hpp"
#include "filter_call.hpp"

namespace rt {
namespace {

__global__ void select_difference_kernel(uint32_t n, const double* __restrict__ a, const double* __restrict__ b, const double* __restrict__ fa,
                                         const double* __restrict__ fb, const double* __restrict__ na, const double* __restrict__ nb,
                                         double* __restrict__ out_d) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; // one thread per pixel
    if (i >= n) return;
    const size_t o = size_t(i) * 3;
    out_d[i] = select_difference(select_cross_error(fa + o, fb + o, a + o, b + o), select_cross_error(na + o, nb + o, a + o, b + o));
}

constexpr int SELECT_BLOCK = int(SELECT_TILE * SELECT_TILE);

__global__ __launch_bounds__(SELECT_BLOCK) void select_blend_kernel(uint32_t width, uint32_t height, SelectParams prm, const double* __restrict__ d,
                                                                    const double* __restrict__ fa, const double* __restrict__ fb,
                                                                    const double* __restrict__ na, const double* __restrict__ nb,
                                                                    double* __restrict__ out, uint8_t* __restrict__ out_rgba8,
                                                                    double* __restrict__ out_blend, double* __restrict__ out_feature,
                                                                    double* __restrict__ out_nlm, double* __restrict__ out_error) {
    extern __shared__ __attribute__((aligned(16))) double select_lds[];
    constexpr int T = int(SELECT_TILE);
    const int s = int(prm.s), t = int(prm.t), halo = s + t;
    const int E = T + 2 * halo, M = T + 2 * t; // the staged region's side, the side of m's region
    double* Dl = select_lds;                    // [E][E] d
    double* Rl = Dl + E * E;                    // [E][M] its row sums
    double* Ml = Rl + E * M;                    // [M][M] m
    double* Ql = Ml + M * M;                    // [M][T] m's row sums
    const int x0 = int(blockIdx.x) * T, y0 = int(blockIdx.y) * T;
    const int tid = int(threadIdx.x);

    for (int i = tid; i < E * E; i += SELECT_BLOCK) {
        const int ey = i / E, ex = i - ey * E;
        Dl[i] = d[size_t(nlm_clamp(y0 - halo, ey, height)) * width + nlm_clamp(x0 - halo, ex, width)];
    }
    __syncthreads();
    for (int i = tid; i < E * M; i += SELECT_BLOCK) {
        const int ey = i / M, mx = i - ey * M;
        double sum = 0.0;
        for (int n = 0; n <= 2 * s; ++n) sum = sum + Dl[ey * E + mx + n]; // mx + 2s < E
        Rl[i] = sum;
    }
    __syncthreads();
    for (int i = tid; i < M * M; i += SELECT_BLOCK) {
        const int my = i / M, mx = i - my * M;
        double sum = 0.0;
        for (int n = 0; n <= 2 * s; ++n) sum = sum + Rl[(my + n) * M + mx]; // my + 2s < E
        Ml[i] = select_choice(sum, prm.threshold);
    }
    __syncthreads();
    // m at region index i of an axis: of the nearest pixel inside the image, which lies in the region too (the tile starts inside the image)
    for (int i = tid; i < M * T; i += SELECT_BLOCK) {
        const int my = i / T, px = i - my * T;
        double sum = 0.0;
        for (int n = 0; n <= 2 * t; ++n) sum = sum + Ml[my * M + (int(nlm_clamp(x0 - t, px + n, width)) - (x0 - t))];
        Ql[i] = sum;
    }
    __syncthreads();
    const int px = tid % T, py = tid / T;
    const uint32_t x = uint32_t(x0 + px), y = uint32_t(y0 + py);
    if (x >= width || y >= height) return;
    double sum = 0.0;
    for (int n = 0; n <= 2 * t; ++n) sum = sum + Ql[(int(nlm_clamp(y0 - t, py + n, height)) - (y0 - t)) * T + px];
    const double beta = select_beta(sum, prm.blend_taps);
    const size_t p = size_t(y) * width + x, o = p * 3;
    out_blend[p] = beta;
    for (int ch = 0; ch < 3; ++ch) {
        const double f = nlm_mean(fa[o + ch], fb[o + ch]), n = nlm_mean(na[o + ch], nb[o + ch]);
        const double c = select_blend(beta, n, f);
        out_feature[o + ch] = f;
        out_nlm[o + ch] = n;
        out[o + ch] = c;
        out_error[o + ch] = nlm_error(select_blend(beta, na[o + ch], fa[o + ch]), select_blend(beta, nb[o + ch], fb[o + ch]));
        out_rgba8[p * 4 + ch] = denoise_quantise(c);
    }
    out_rgba8[p * 4 + 3] = 255;
}

} // namespace

int select_device(uint32_t width, uint32_t height, const double* half_a, const double* half_b, const double* var_a, const double* var_b,
                  const double* albedo, const double* normal, const double* depth, const double* alpha, uint32_t iterations, const DenoiseParams& dn,
                  const NlmParams& nl, const SelectParams& sel, double* out_linear_rgb, uint8_t* out_rgba8, double* out_blend, double* out_feature_rgb,
                  double* out_nlm_rgb, double* out_error_rgb, double* kernel_ms) {
    FilterCall fc;
    if (int rc = fc.open("denoise_select", width, height)) return rc;
    const size_t npx = fc.npx;
    const bool has_var = var_a != nullptr;
    DevBuf<double> d_a, d_b, d_va, d_vb, d_albedo, d_normal, d_depth, d_alpha, d_ca[2], d_cb[2], d_v[2], d_na, d_nb, d_d, d_out, d_blend, d_feature, d_nlm, d_err;
    DevBuf<uint8_t> d_rgba;
    fc.upload(d_a, half_a, 3);
    fc.upload(d_b, half_b, 3);
    if (has_var) {
        fc.upload(d_va, var_a, 3);
        fc.upload(d_vb, var_b, 3);
    } else {
        fc.alloc(d_va, 3); // the pair variance of the non-local-means step: one array for both guides
    }
    fc.upload(d_albedo, albedo, 3);
    fc.upload(d_normal, normal, 3);
    fc.upload(d_depth, depth, 1);
    fc.upload(d_alpha, alpha, 1);
    for (int k = 0; k < 2; ++k) {
        fc.alloc(d_ca[k], 3);
        fc.alloc(d_cb[k], 3);
        if (has_var) fc.alloc(d_v[k], 3); // the filtered variances are not an output: the two runs share their buffers
    }
    fc.alloc(d_na, 3);
    fc.alloc(d_nb, 3);
    fc.alloc(d_d, 1);
    fc.alloc(d_out, 3);
    fc.alloc(d_blend, 1);
    fc.alloc(d_feature, 3);
    fc.alloc(d_nlm, 3);
    fc.alloc(d_err, 3);
    fc.alloc(d_rgba, 4); // the à-trous runs' RGBA8, then the call's
    const char* const at = fc.at.c_str();
    NlmPlan plan;
    if (int rc = nlm_plan_device(at, nl, plan)) return rc;
    const size_t lds_bytes = select_lds_bytes(sel.s, sel.t);
    HIP_TRY_AS(at, hipFuncSetAttribute(reinterpret_cast<const void*>(select_blend_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds_bytes)));

    const hipStream_t stream = fc.stream;
    double* const ca[2] = {d_ca[0].p, d_ca[1].p};
    double* const cb[2] = {d_cb[0].p, d_cb[1].p};
    double* const v[2] = {d_v[0].p, d_v[1].p};
    uint8_t* const no_h[2] = {nullptr, nullptr};
    int out_a = 0, out_b = 0;
    if (int rc = fc.start()) return rc;
    if (int rc = atrous_passes_device(width, height, d_a.p, has_var ? d_va.p : nullptr, nullptr, d_albedo.p, d_normal.p, d_depth.p, d_alpha.p, iterations, dn,
                                      ca, v, no_h, d_rgba.p, nullptr, stream, out_a)) return rc;
    if (int rc = atrous_passes_device(width, height, d_b.p, has_var ? d_vb.p : nullptr, nullptr, d_albedo.p, d_normal.p, d_depth.p, d_alpha.p, iterations, dn,
                                      cb, v, no_h, d_rgba.p, nullptr, stream, out_b)) return rc;
    if (int rc = nlm_passes_device(at, width, height, d_a.p, d_b.p, has_var ? d_va.p : nullptr, has_var ? d_vb.p : nullptr, has_var ? nullptr : d_va.p, nl,
                                   plan, d_na.p, d_nb.p, nullptr, nullptr, nullptr, stream)) return rc;
    const double *fa = ca[out_a], *fb = cb[out_b];
    hipLaunchKernelGGL(select_difference_kernel, dim3(uint32_t((npx + 255) / 256)), dim3(256), 0, stream, uint32_t(npx), d_a.p, d_b.p, fa, fb, d_na.p,
                       d_nb.p, d_d.p);
    const dim3 tiles((width + SELECT_TILE - 1) / SELECT_TILE, (height + SELECT_TILE - 1) / SELECT_TILE);
    hipLaunchKernelGGL(select_blend_kernel, tiles, dim3(SELECT_BLOCK), lds_bytes, stream, width, height, sel, d_d.p, fa, fb, d_na.p, d_nb.p, d_out.p,
                       d_rgba.p, d_blend.p, d_feature.p, d_nlm.p, d_err.p);
    HIP_TRY_AS(at, hipGetLastError());
    if (int rc = fc.finish(kernel_ms)) return rc;
    fc.copy_out(out_linear_rgb, d_out, 3);
    fc.copy_out(out_rgba8, d_rgba, 4);
    fc.copy_out(out_blend, d_blend, 1);
    fc.copy_out(out_feature_rgb, d_feature, 3);
    fc.copy_out(out_nlm_rgb, d_nlm, 3);
    fc.copy_out(out_error_rgb, d_err, 3);
    return fc.rc;
}

} // namespace rt
