// Host harness of rttnw_amd/csrc/denoise.hpp: rttnw_denoise's passes with the functions the device kernels (denoise.hip) call, pixel by
// pixel, behind a C interface for tests/test_denoise_cpu.py and tests/test_gpu_denoise.py.
#include "../../rttnw_amd/csrc/denoise.hpp"
#include <vector>

extern "C" int dh_denoise(uint32_t w, uint32_t h, const double* colour, const double* variance, const double* albedo, const double* normal,
                          const double* depth, const double* alpha, uint32_t iterations, double sigma_luminance, double sigma_normal,
                          double sigma_depth, double* out_colour, uint8_t* out_rgba8, double* out_variance) {
    if (iterations > rt::DENOISE_MAX_ITERATIONS) return -1;
    const size_t n = size_t(w) * h;
    const rt::DenoiseParams prm = rt::denoise_params(sigma_luminance, sigma_normal, sigma_depth, variance != nullptr);
    std::vector<double> c(colour, colour + n * 3), v, c2(n * 3), v2;
    if (variance) { v.assign(variance, variance + n * 3); v2.resize(n * 3); }
    for (size_t i = 0; iterations > 0 && i < n * 3; ++i) {
        c[i] = rt::denoise_demodulate(colour[i], albedo[i], alpha[i / 3]);
        if (variance) v[i] = rt::denoise_demodulate_variance(variance[i], albedo[i], alpha[i / 3]);
    }
    for (uint32_t it = 0; it < iterations; ++it) {
        const rt::DenoiseView view{w, h, c.data(), variance ? v.data() : nullptr, normal, depth, alpha};
        for (uint32_t y = 0; y < h; ++y)
            for (uint32_t x = 0; x < w; ++x) {
                const size_t o = (size_t(y) * w + x) * 3;
                double dummy[3];
                rt::denoise_filter_pixel(view, prm, x, y, 1u << it, &c2[o], variance ? &v2[o] : dummy);
            }
        c.swap(c2);
        v.swap(v2);
    }
    for (size_t i = 0; i < n * 3; ++i) {
        const double r = iterations > 0 ? rt::denoise_remodulate(c[i], albedo[i], alpha[i / 3]) : c[i];
        if (out_colour) out_colour[i] = r;
        if (out_rgba8) out_rgba8[i / 3 * 4 + i % 3] = rt::denoise_quantise(r);
        if (out_variance && variance) out_variance[i] = iterations > 0 ? rt::denoise_remodulate_variance(v[i], albedo[i], alpha[i / 3]) : v[i];
    }
    for (size_t i = 0; out_rgba8 && i < n; ++i) out_rgba8[i * 4 + 3] = 255;
    return 0;
}
