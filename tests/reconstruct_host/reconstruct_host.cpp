// Host harness of rttnw_amd/csrc/reconstruct.hpp: rttnw_reconstruct's passes with the functions the device kernels (reconstruct.hip) call, pixel
// by pixel, behind a C interface for tests/test_reconstruct_cpu.py and tests/test_gpu_reconstruct.py.
#include "../../rttnw_amd/csrc/reconstruct.hpp"
#include <vector>

extern "C" int rh_reconstruct(uint32_t w, uint32_t h, const double* colour, const double* variance, const uint8_t* valid, const double* albedo,
                              const double* normal, const double* depth, const double* alpha, uint32_t iterations, double sigma_luminance,
                              double sigma_normal, double sigma_depth, double* out_colour, uint8_t* out_rgba8, double* out_variance, uint8_t* out_valid) {
    if (iterations > rt::DENOISE_MAX_ITERATIONS) return -1;
    const size_t n = size_t(w) * h;
    const rt::DenoiseParams prm = rt::denoise_params(sigma_luminance, sigma_normal, sigma_depth, variance != nullptr);
    std::vector<double> c(n * 3), v(variance ? n * 3 : 0), c2(n * 3), v2(variance ? n * 3 : 0);
    std::vector<uint8_t> hd(n), hd2(n);
    const double* colour_now = colour;
    const double* variance_now = variance;
    const uint8_t* holds_now = valid;
    if (iterations > 0) {
        for (size_t i = 0; i < n; ++i)
            hd[i] = rt::reconstruct_prepare_pixel(valid[i] != 0, colour + i * 3, variance ? variance + i * 3 : nullptr, albedo + i * 3, alpha[i], &c[i * 3],
                                                  variance ? &v[i * 3] : nullptr);
        for (uint32_t it = 0; it < iterations; ++it) {
            const rt::ReconstructView view{{w, h, c.data(), variance ? v.data() : nullptr, normal, depth, alpha}, hd.data()};
            for (uint32_t y = 0; y < h; ++y)
                for (uint32_t x = 0; x < w; ++x) {
                    const size_t p = size_t(y) * w + x;
                    double dummy[3];
                    hd2[p] = rt::reconstruct_filter_pixel(view, prm, x, y, 1u << it, &c2[p * 3], variance ? &v2[p * 3] : dummy);
                }
            c.swap(c2);
            v.swap(v2);
            hd.swap(hd2);
        }
        colour_now = c.data();
        variance_now = variance ? v.data() : nullptr;
        holds_now = hd.data();
    }
    for (size_t i = 0; i < n; ++i) {
        double oc[3], ov[3];
        uint8_t rgba[4];
        const uint8_t ok = rt::reconstruct_finish_pixel(holds_now[i] != 0, iterations > 0, colour_now + i * 3, variance_now ? variance_now + i * 3 : nullptr,
                                                        albedo + i * 3, alpha[i], oc, rgba, variance_now ? ov : nullptr);
        for (int ch = 0; ch < 3; ++ch) {
            if (out_colour) out_colour[i * 3 + ch] = oc[ch];
            if (out_variance && variance) out_variance[i * 3 + ch] = ov[ch];
        }
        for (int ch = 0; ch < 4 && out_rgba8; ++ch) out_rgba8[i * 4 + ch] = rgba[ch];
        if (out_valid) out_valid[i] = ok;
    }
    return 0;
}
