// Host harness of rttnw_amd/csrc/select.hpp: rttnw_denoise_select with the functions the device kernels (select.hip) call, in the order the
// header states, over the host builds of the two filters (tests/denoise_host, tests/nlm_host: their sources are compiled into this library, so the
// filtered halves are those harnesses' bits), behind a C interface for tests/test_select_cpu.py and tests/test_gpu_select.py.  Whole-image maps
// in place of the device's tiles: d, its row sums, m, m's row sums, beta.
#include "../../rttnw_amd/csrc/select.hpp"
#include "../denoise_host/denoise_host.cpp"
#include "../nlm_host/nlm_host.cpp"

namespace {

// out(x, y) = sum over oy = -radius .. radius, top to bottom, of (sum over ox = -radius .. radius, left to right, of in(clamp(x + ox), clamp(y + oy)))
std::vector<double> window_sums(uint32_t w, uint32_t h, const std::vector<double>& in, int radius) {
    std::vector<double> rows(in.size()), out(in.size());
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) {
            double sum = 0.0;
            for (int ox = -radius; ox <= radius; ++ox) sum = sum + in[size_t(y) * w + rt::nlm_clamp(int(x), ox, w)];
            rows[size_t(y) * w + x] = sum;
        }
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) {
            double sum = 0.0;
            for (int oy = -radius; oy <= radius; ++oy) sum = sum + rows[size_t(rt::nlm_clamp(int(y), oy, h)) * w + x];
            out[size_t(y) * w + x] = sum;
        }
    return out;
}

} // namespace

extern "C" int sh_denoise_select(uint32_t w, uint32_t h, const double* a, const double* b, const double* var_a, const double* var_b, const double* albedo,
                                 const double* normal, const double* depth, const double* alpha, uint32_t iterations, double sigma_luminance,
                                 double sigma_normal, double sigma_depth, uint32_t search_radius, uint32_t patch_radius, double k, uint32_t error_radius,
                                 uint32_t blend_radius, double margin, uint32_t use_default_margin, double* out, uint8_t* out_rgba8, double* out_blend,
                                 double* out_feature, double* out_nlm, double* out_error) {
    if (error_radius > rt::SELECT_MAX_ERROR_RADIUS || blend_radius > rt::SELECT_MAX_BLEND_RADIUS) return -1;
    if (!use_default_margin && !(margin >= -2.0 && margin <= 2.0)) return -1;
    const rt::SelectParams prm = rt::select_params(error_radius, blend_radius, margin, use_default_margin != 0);
    const size_t n = size_t(w) * h;
    std::vector<double> fa(n * 3), fb(n * 3), na(n * 3), nb(n * 3), d(n);
    if (dh_denoise(w, h, a, var_a, albedo, normal, depth, alpha, iterations, sigma_luminance, sigma_normal, sigma_depth, fa.data(), nullptr, nullptr)) return -1;
    if (dh_denoise(w, h, b, var_b, albedo, normal, depth, alpha, iterations, sigma_luminance, sigma_normal, sigma_depth, fb.data(), nullptr, nullptr)) return -1;
    if (nh_denoise_nlm(w, h, a, b, var_a, var_b, search_radius, patch_radius, k, nullptr, nullptr, na.data(), nb.data(), nullptr)) return -1;
    for (size_t p = 0; p < n; ++p) {
        const size_t o = p * 3;
        d[p] = rt::select_difference(rt::select_cross_error(&fa[o], &fb[o], a + o, b + o), rt::select_cross_error(&na[o], &nb[o], a + o, b + o));
    }
    std::vector<double> m = window_sums(w, h, d, int(prm.s));
    for (size_t p = 0; p < n; ++p) m[p] = rt::select_choice(m[p], prm.threshold);
    const std::vector<double> sums = window_sums(w, h, m, int(prm.t));
    for (size_t p = 0; p < n; ++p) {
        const double beta = rt::select_beta(sums[p], prm.blend_taps);
        if (out_blend) out_blend[p] = beta;
        for (size_t i = p * 3; i < p * 3 + 3; ++i) {
            const double f = rt::nlm_mean(fa[i], fb[i]), nl = rt::nlm_mean(na[i], nb[i]);
            const double c = rt::select_blend(beta, nl, f);
            if (out) out[i] = c;
            if (out_rgba8) out_rgba8[p * 4 + (i - p * 3)] = rt::denoise_quantise(c);
            if (out_feature) out_feature[i] = f;
            if (out_nlm) out_nlm[i] = nl;
            if (out_error) out_error[i] = rt::nlm_error(rt::select_blend(beta, na[i], fa[i]), rt::select_blend(beta, nb[i], fb[i]));
        }
        if (out_rgba8) out_rgba8[p * 4 + 3] = 255;
    }
    return 0;
}
