// regress.hip — the device half of rttnw_denoise_regress (include/rttnw_hip.h) around the arithmetic of regress.hpp, double throughout:
//   regress_prepare_kernel   one thread per pixel: the demodulated halves and variances (with demodulate) and the pixel's 64-byte feature
//                            record (with a feature mask): albedo, normal, z = depth / alpha, alpha — a candidate's features are one line
//   regress_variance_kernel  the pair variance of the (demodulated) halves, only when the caller gave none
//   regress_filter_kernel    nlm.hip's filter kernel with the accumulation replaced: one block per TxT tile and direction (blockIdx.z 0: guide B
//                            weighs half A; 1: guide A weighs half B), one thread per pixel, guide and variance staged in LDS with a halo of
//                            r + f, every delta of the tile formed once per offset, two barriers per offset.  Each thread keeps the running
//                            sums of regress.hpp in registers — the kernel is specialised on the feature mask, so A, b, C and L have
//                            compile-time indices — and solves its 7x7 system once, after the loop.
//   regress_finish_kernel    the mean of the two fitted halves, its RGBA8, the error estimate and the fit count
// The 60 running doubles of d = 7 are 120 VGPRs before the loop's own: they do not fit the 128 registers of a 1024-thread block, so masks
// with d >= 6 run the 16-pixel tile (256 threads) at every radius (regress.hpp regress_tile_large); KERNELS.md has the registers per mask.
// The host half is split as nlm.hip's: regress_plan_device (the filter instantiation, its tile, its LDS admitted), regress_passes_device (the
// kernels enqueued over device pointers: nothing allocated, copied or waited for — the rttnw_svgf handle's spatial stage calls it, svgf.hip) and
// regress_device, the blocking call on host arrays around the two.
#include "feature_api.hpp"
#include "filter_call.hpp"
#include "regress.hpp"

namespace rt {
namespace {

__global__ void regress_prepare_kernel(uint32_t n, uint32_t mask, bool demodulate, const double* __restrict__ a, const double* __restrict__ b,
                                       const double* __restrict__ va, const double* __restrict__ vb, const double* __restrict__ albedo,
                                       const double* __restrict__ normal, const double* __restrict__ depth, const double* __restrict__ alpha,
                                       double* __restrict__ wa, double* __restrict__ wb, double* __restrict__ wva, double* __restrict__ wvb,
                                       RegressRecord* __restrict__ rec) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; // one thread per pixel
    if (p >= n) return;
    if (demodulate) {
        const double al = alpha[p];
        for (uint32_t ch = 0; ch < 3u; ++ch) {
            const size_t i = size_t(p) * 3 + ch;
            const double alb = albedo[i];
            wa[i] = denoise_demodulate(a[i], alb, al);
            wb[i] = denoise_demodulate(b[i], alb, al);
            if (va) {
                wva[i] = denoise_demodulate_variance(va[i], alb, al);
                wvb[i] = denoise_demodulate_variance(vb[i], alb, al);
            }
        }
    }
    if (mask != 0u) rec[p] = regress_record(mask, albedo, normal, depth, alpha, p);
}

__global__ void regress_variance_kernel(uint32_t width, uint32_t height, const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; // one thread per channel value
    if (i >= width * height * 3u) return;
    const uint32_t pixel = i / 3u;
    out[i] = nlm_pair_variance(width, height, a, b, pixel % width, pixel / width, int(i - pixel * 3u));
}

template <int T, uint32_t M> // the tile's side (one thread per pixel of the tile) and the feature mask
__global__ __launch_bounds__(T * T) void regress_filter_kernel(NlmView in, RegressParams rp, const RegressRecord* __restrict__ rec,
                                                               const double* __restrict__ albedo, const double* __restrict__ alpha,
                                                               double* __restrict__ out_a, double* __restrict__ out_b, uint8_t* __restrict__ fit_a,
                                                               uint8_t* __restrict__ fit_b) {
    extern __shared__ __attribute__((aligned(16))) double regress_lds[];
    constexpr int BLOCK = T * T, D = regress_dim(M);
    const NlmParams prm = rp.nlm;
    const int r = int(prm.r), f = int(prm.f), halo = r + f;
    const int E = T + 2 * halo, P = T + 2 * f, plane = E * E; // the staged region's side, the delta region's side
    double* G = regress_lds;                                  // [3][E][E] the guide
    double* V = regress_lds + 3 * plane;                      // [3][E][E] its variance
    double* Dl = regress_lds + 6 * plane;                     // [P][P] delta(x, o) of the current offset
    double* Rl = Dl + P * P;                                  // [P][T] the row sums
    const bool second = blockIdx.z != 0;
    const double* __restrict__ guide = second ? in.a : in.b;
    const double* __restrict__ var = second ? in.var_a : in.var_b;
    const double* __restrict__ src = second ? in.b : in.a;
    const int x0 = int(blockIdx.x) * T, y0 = int(blockIdx.y) * T;
    const int tid = int(threadIdx.x);

    for (int i = tid; i < plane; i += BLOCK) {
        const int ey = i / E, ex = i - ey * E;
        const size_t q = (size_t(nlm_clamp(y0 - halo, ey, in.height)) * in.width + nlm_clamp(x0 - halo, ex, in.width)) * 3;
        for (int ch = 0; ch < 3; ++ch) {
            G[ch * plane + i] = guide[q + ch];
            V[ch * plane + i] = var[q + ch];
        }
    }
    __syncthreads();

    const int px = tid % T, py = tid / T;
    const bool inside = uint32_t(x0 + px) < in.width && uint32_t(y0 + py) < in.height; // a thread off the image only helps with the tile's deltas
    const size_t p = inside ? size_t(y0 + py) * in.width + size_t(x0 + px) : 0;
    RegressRecord centre = {};
    bool first_order = false; // the pixel's mask m is M, or 0 where its alpha == 0
    if (M != 0u && inside) {
        centre = rec[p];
        first_order = centre.alpha != 0.0;
    }
    RegressSums<D> S;
    S.clear();
    for (int oy = -r; oy <= r; ++oy)
        for (int ox = -r; ox <= r; ++ox) {
            double w = 1.0; // the centre offset
            if (ox != 0 || oy != 0) { // (uniform over the block: the barriers below are reached by all of its threads or by none)
                for (int i = tid; i < P * P; i += BLOCK) {
                    const int dy = i / P, dx = i - dy * P;
                    const int xs = (dy + r) * E + dx + r, qs = xs + oy * E + ox; // 0 <= dy + r + oy, dx + r + ox < E
                    const double d0 = nlm_delta_channel(G[xs], G[qs], V[xs], V[qs], prm.k2);
                    const double d1 = nlm_delta_channel(G[plane + xs], G[plane + qs], V[plane + xs], V[plane + qs], prm.k2);
                    const double d2 = nlm_delta_channel(G[2 * plane + xs], G[2 * plane + qs], V[2 * plane + xs], V[2 * plane + qs], prm.k2);
                    Dl[i] = nlm_delta(d0, d1, d2);
                }
                __syncthreads();
                for (int i = tid; i < P * T; i += BLOCK) {
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
            if (!inside) continue; // (behind the offset's barriers)
            const size_t q = size_t(nlm_clamp(y0 + py, oy, in.height)) * in.width + nlm_clamp(x0 + px, ox, in.width); // clamped: inside the image
            const double y[3] = {src[q * 3], src[q * 3 + 1], src[q * 3 + 2]};
            if (M != 0u && first_order) {
                const RegressRecord& cand = rec[q];
                if (cand.alpha == 0.0) continue; // a dropped candidate enters no sum
                double x[D > 0 ? D : 1];
                regress_x<M>(centre, cand, x);
                S.add_zero_order(w, y);
                S.add_first_order(w, x, y);
            } else {
                S.add_zero_order(w, y);
            }
        }
    if (!inside) return;
    double value[3];
    const bool fitted = regress_solve<D>(S, rp.ridge, first_order, value);
    double* dst = (second ? out_b : out_a) + p * 3;
    for (int ch = 0; ch < 3; ++ch) dst[ch] = rp.demodulate ? denoise_remodulate(value[ch], albedo[p * 3 + ch], alpha[p]) : value[ch];
    (second ? fit_b : fit_a)[p] = fitted ? 1 : 0;
}

__global__ void regress_finish_kernel(uint32_t n, const double* __restrict__ fa, const double* __restrict__ fb, const uint8_t* __restrict__ fit_a,
                                      const uint8_t* __restrict__ fit_b, double* __restrict__ out, uint8_t* __restrict__ out_rgba8,
                                      double* __restrict__ out_error, double* __restrict__ out_fit) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; // one thread per channel value
    if (i >= n * 3u) return;
    const uint32_t pixel = i / 3u, ch = i - pixel * 3u;
    const double c = nlm_mean(fa[i], fb[i]);
    out[i] = c;
    out_error[i] = nlm_error(fa[i], fb[i]);
    out_rgba8[pixel * 4u + ch] = denoise_quantise(c);
    if (ch == 0u) {
        out_rgba8[pixel * 4u + 3u] = 255;
        out_fit[pixel] = double(fit_a[pixel] + fit_b[pixel]);
    }
}

using RegressFilter = decltype(RegressPlan::filter);
// (a mask that never takes the large tile has no large instantiation: its slot holds mask 0's, which is never launched for it)
template <uint32_t M> constexpr RegressFilter regress_filter(bool large) {
    return large ? regress_filter_kernel<int(NLM_TILE_LARGE), regress_mask_fits_large_tile(M) ? M : 0u> : regress_filter_kernel<int(NLM_TILE_SMALL), M>;
}

} // namespace

// The filter kernel of the call's mask and radii, its tile, and its dynamic LDS admitted: before the caller starts its clock
int regress_plan_device(const char* at, const RegressParams& prm, RegressPlan& plan) {
    const uint32_t mask = prm.features;
    const bool large = regress_tile_large(mask, prm.nlm.r, prm.nlm.f);
    static const RegressFilter LARGE[8] = {regress_filter<0>(true), regress_filter<1>(true), regress_filter<2>(true), regress_filter<3>(true),
                                               regress_filter<4>(true), regress_filter<5>(true), regress_filter<6>(true), regress_filter<7>(true)};
    static const RegressFilter SMALL[8] = {regress_filter<0>(false), regress_filter<1>(false), regress_filter<2>(false), regress_filter<3>(false),
                                               regress_filter<4>(false), regress_filter<5>(false), regress_filter<6>(false), regress_filter<7>(false)};
    plan.filter = large ? LARGE[mask] : SMALL[mask];
    plan.tile = large ? NLM_TILE_LARGE : NLM_TILE_SMALL;
    plan.lds_bytes = nlm_lds_bytes(plan.tile, prm.nlm.r, prm.nlm.f);
    HIP_TRY_AS(at, hipFuncSetAttribute(reinterpret_cast<const void*>(plan.filter), hipFuncAttributeMaxDynamicSharedMemorySize, int(plan.lds_bytes)));
    return RTTNW_OK;
}

// The kernels alone, enqueued on `stream` over buffers that are already on the device: nothing allocated, nothing copied, no wait
int regress_passes_device(const char* at, uint32_t width, uint32_t height, const double* d_a, const double* d_b, const double* d_var_a, const double* d_var_b,
                          const double* d_albedo, const double* d_normal, const double* d_depth, const double* d_alpha, const RegressParams& prm,
                          const RegressPlan& plan, const RegressWork& k, hipStream_t stream) {
    const size_t npx = size_t(width) * height;
    const uint32_t mask = prm.features;
    const bool has_var = d_var_a != nullptr, demodulate = prm.demodulate != 0;
    const dim3 flat_block(256), pixel_grid(uint32_t((npx + 255) / 256)), value_grid(uint32_t((npx * 3 + 255) / 256));
    const dim3 tiles((width + plan.tile - 1) / plan.tile, (height + plan.tile - 1) / plan.tile, 2);
    if (demodulate || mask != 0u)
        hipLaunchKernelGGL(regress_prepare_kernel, pixel_grid, flat_block, 0, stream, uint32_t(npx), mask, demodulate, d_a, d_b, d_var_a, d_var_b, d_albedo,
                           d_normal, d_depth, d_alpha, k.wa, k.wb, k.wva, k.wvb, k.rec);
    const double* w_a = demodulate ? k.wa : d_a;
    const double* w_b = demodulate ? k.wb : d_b;
    const double* w_va = !has_var ? k.pair : demodulate ? k.wva : d_var_a;
    const double* w_vb = !has_var ? k.pair : demodulate ? k.wvb : d_var_b;
    if (!has_var) hipLaunchKernelGGL(regress_variance_kernel, value_grid, flat_block, 0, stream, width, height, w_a, w_b, k.pair);
    const NlmView view{width, height, w_a, w_b, w_va, w_vb};
    hipLaunchKernelGGL(plan.filter, tiles, dim3(plan.tile * plan.tile), plan.lds_bytes, stream, view, prm, (const RegressRecord*)k.rec, d_albedo, d_alpha, k.fa,
                       k.fb, k.fit_a, k.fit_b);
    hipLaunchKernelGGL(regress_finish_kernel, value_grid, flat_block, 0, stream, uint32_t(npx), (const double*)k.fa, (const double*)k.fb,
                       (const uint8_t*)k.fit_a, (const uint8_t*)k.fit_b, k.out, k.rgba, k.err, k.fit);
    HIP_TRY_AS(at, hipGetLastError());
    return RTTNW_OK;
}

// rttnw_denoise_regress's device half: the caller's arrays and the workspace on the device, the kernels between two events, the outputs the
// caller asked for.
int regress_device(uint32_t width, uint32_t height, const double* half_a, const double* half_b, const double* var_a, const double* var_b,
                   const double* albedo, const double* normal, const double* depth, const double* alpha, const RegressParams& prm,
                   double* out_linear_rgb, uint8_t* out_rgba8, double* out_half_a, double* out_half_b, double* out_error_rgb, double* out_fit,
                   double* kernel_ms) {
    FilterCall fc;
    if (int rc = fc.open("denoise_regress", width, height)) return rc;
    const uint32_t mask = prm.features;
    const bool has_var = var_a != nullptr, demodulate = prm.demodulate != 0;
    DevBuf<double> d_a, d_b, d_va, d_vb, d_albedo, d_normal, d_depth, d_alpha, d_wa, d_wb, d_wva, d_wvb, d_pair, d_fa, d_fb, d_out, d_err, d_fit;
    DevBuf<uint8_t> d_rgba, d_fit_a, d_fit_b;
    DevBuf<RegressRecord> d_rec;
    fc.upload(d_a, half_a, 3);
    fc.upload(d_b, half_b, 3);
    if (has_var) {
        fc.upload(d_va, var_a, 3);
        fc.upload(d_vb, var_b, 3);
    } else {
        fc.alloc(d_pair, 3); // the pair variance: one array for both guides
    }
    // the feature arrays the call reads: each one its mask bit asks for, the albedo for the demodulation, alpha for either
    if ((mask & REGRESS_ALBEDO) || demodulate) fc.upload(d_albedo, albedo, 3);
    if (mask & REGRESS_NORMAL) fc.upload(d_normal, normal, 3);
    if (mask & REGRESS_DEPTH) fc.upload(d_depth, depth, 1);
    if (mask != 0u || demodulate) fc.upload(d_alpha, alpha, 1);
    if (demodulate) {
        fc.alloc(d_wa, 3);
        fc.alloc(d_wb, 3);
        if (has_var) {
            fc.alloc(d_wva, 3);
            fc.alloc(d_wvb, 3);
        }
    }
    if (mask != 0u) fc.alloc(d_rec, 1);
    fc.alloc(d_fa, 3);
    fc.alloc(d_fb, 3);
    fc.alloc(d_out, 3);
    fc.alloc(d_err, 3);
    fc.alloc(d_fit, 1);
    fc.alloc(d_rgba, 4);
    fc.alloc(d_fit_a, 1);
    fc.alloc(d_fit_b, 1);
    if (fc.rc) return fc.rc;

    RegressPlan plan;
    if (int rc = regress_plan_device(fc.at.c_str(), prm, plan)) return rc; // before the clock starts
    const RegressWork work{d_wa.p, d_wb.p, d_wva.p, d_wvb.p, d_pair.p, d_rec.p, d_fa.p, d_fb.p, d_fit_a.p, d_fit_b.p, d_out.p, d_rgba.p, d_err.p, d_fit.p};
    if (int rc = fc.start()) return rc;
    if (int rc = regress_passes_device(fc.at.c_str(), width, height, d_a.p, d_b.p, d_va.p, d_vb.p, d_albedo.p, d_normal.p, d_depth.p, d_alpha.p, prm, plan, work,
                                       fc.stream)) return rc;
    if (int rc = fc.finish(kernel_ms)) return rc;
    fc.copy_out(out_linear_rgb, d_out, 3);
    fc.copy_out(out_rgba8, d_rgba, 4);
    fc.copy_out(out_half_a, d_fa, 3);
    fc.copy_out(out_half_b, d_fb, 3);
    fc.copy_out(out_error_rgb, d_err, 3);
    fc.copy_out(out_fit, d_fit, 1);
    return fc.rc;
}

} // namespace rt
