// Host harness of rttnw_amd/csrc/nlm.hpp: rttnw_denoise_nlm with the functions the device kernels (nlm.hip) call, in the order the header
// states, behind a C interface for tests/test_nlm_cpu.py and tests/test_gpu_nlm.py.  Whole-image maps per offset in place of the device's
// tiles: delta over the image and its patch halo, the row sums, then each pixel's column sum.
#include "../../rttnw_amd/csrc/nlm.hpp"
#include <vector>

namespace {

// `src` filtered by the weights of `guide` with variance `var`: out w*h*3
void cross_filter(uint32_t w, uint32_t h, const double* guide, const double* var, const double* src, const rt::NlmParams& prm, double* out) {
    const int r = int(prm.r), f = int(prm.f), pw = int(w) + 2 * f, ph = int(h) + 2 * f;
    const size_t n = size_t(w) * h;
    std::vector<double> delta(size_t(pw) * ph), rows(size_t(w) * ph), sum_w(n, 0.0), sum_c(n * 3, 0.0);
    for (int oy = -r; oy <= r; ++oy)
        for (int ox = -r; ox <= r; ++ox) {
            const bool centre = ox == 0 && oy == 0;
            for (int ey = 0; !centre && ey < ph; ++ey)
                for (int ex = 0; ex < pw; ++ex) { // the extended coordinate (ex - f, ey - f)
                    const size_t x = (size_t(rt::nlm_clamp(ey - f, 0, h)) * w + rt::nlm_clamp(ex - f, 0, w)) * 3;
                    const size_t q = (size_t(rt::nlm_clamp(ey - f, oy, h)) * w + rt::nlm_clamp(ex - f, ox, w)) * 3;
                    double d[3];
                    for (int ch = 0; ch < 3; ++ch) d[ch] = rt::nlm_delta_channel(guide[x + ch], guide[q + ch], var[x + ch], var[q + ch], prm.k2);
                    delta[size_t(ey) * pw + ex] = rt::nlm_delta(d[0], d[1], d[2]);
                }
            for (int ey = 0; !centre && ey < ph; ++ey)
                for (uint32_t x = 0; x < w; ++x) {
                    double sum = 0.0;
                    for (int k = 0; k <= 2 * f; ++k) sum = sum + delta[size_t(ey) * pw + x + k];
                    rows[size_t(ey) * w + x] = sum;
                }
            for (uint32_t y = 0; y < h; ++y)
                for (uint32_t x = 0; x < w; ++x) {
                    double wgt = 1.0;
                    if (!centre) {
                        double column = 0.0;
                        for (int k = 0; k <= 2 * f; ++k) column = column + rows[size_t(y + k) * w + x];
                        wgt = rt::nlm_weight(column, prm.patch_taps);
                    }
                    const size_t p = size_t(y) * w + x;
                    const size_t q = (size_t(rt::nlm_clamp(int(y), oy, h)) * w + rt::nlm_clamp(int(x), ox, w)) * 3;
                    sum_w[p] = sum_w[p] + wgt;
                    for (int ch = 0; ch < 3; ++ch) sum_c[p * 3 + ch] = sum_c[p * 3 + ch] + rt::unfused_mul(wgt, src[q + ch]);
                }
        }
    for (size_t i = 0; i < n * 3; ++i) out[i] = sum_c[i] / sum_w[i / 3];
}

} // namespace

extern "C" int nh_denoise_nlm(uint32_t w, uint32_t h, const double* a, const double* b, const double* var_a, const double* var_b, uint32_t search_radius,
                              uint32_t patch_radius, double k, double* out, uint8_t* out_rgba8, double* out_a, double* out_b, double* out_error) {
    if (search_radius > rt::NLM_MAX_SEARCH_RADIUS || patch_radius > rt::NLM_MAX_PATCH_RADIUS || !(k >= 0.0) || (var_a == nullptr) != (var_b == nullptr)) return -1;
    const rt::NlmParams prm = rt::nlm_params(search_radius, patch_radius, k);
    const size_t n = size_t(w) * h;
    std::vector<double> pair, fa(n * 3), fb(n * 3);
    if (!var_a) {
        pair.resize(n * 3);
        for (size_t i = 0; i < n * 3; ++i) pair[i] = rt::nlm_pair_variance(w, h, a, b, uint32_t(i / 3 % w), uint32_t(i / 3 / w), int(i % 3));
        var_a = var_b = pair.data();
    }
    cross_filter(w, h, b, var_b, a, prm, fa.data());
    cross_filter(w, h, a, var_a, b, prm, fb.data());
    for (size_t i = 0; i < n * 3; ++i) {
        const double c = rt::nlm_mean(fa[i], fb[i]);
        if (out) out[i] = c;
        if (out_rgba8) out_rgba8[i / 3 * 4 + i % 3] = rt::denoise_quantise(c);
        if (out_a) out_a[i] = fa[i];
        if (out_b) out_b[i] = fb[i];
        if (out_error) out_error[i] = rt::nlm_error(fa[i], fb[i]);
    }
    for (size_t i = 0; out_rgba8 && i < n; ++i) out_rgba8[i * 4 + 3] = 255;
    return 0;
}
