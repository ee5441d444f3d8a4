// denoise.hpp — the arithmetic of rttnw_denoise (include/rttnw_hip.h has the contract, DESIGN.md §10b the why), shared by the device
// kernels (denoise.hip) and the host test harness (tests/denoise_host): an edge-avoiding à-trous wavelet filter (Dammertz et al. 2010)
// over the demodulated image, its edge-stopping weights taken from the first-hit feature buffers of rttnw_render_features and, where the
// caller has one, from the variance of the pixel means (the colour stop of SVGF, Schied et al. 2017).
//
// Everything is double.  The weights use + - * /, sqrt, comparisons and integer powers by repeated squaring only — no transcendental
// function — every product goes through unfused_mul() (adaptive.hpp: the device units are built with contraction on), and the 25 taps
// are accumulated row-major over the 5x5.  So the device code, a g++ host build and a tap-ordered numpy restatement produce the same bits
// (tests/test_denoise_cpu.py, tests/test_gpu_denoise.py).
#pragma once
#include "adaptive.hpp"

namespace rt {

constexpr uint32_t DENOISE_MAX_ITERATIONS = 8;
constexpr double DENOISE_ALBEDO_EPS = 1e-3; // a channel is demodulated where its albedo exceeds this
constexpr double DENOISE_TINY = 1e-12;      // keeps the weights' denominators positive
// The library defaults (a sigma of 0 in rttnw_denoise_params); DESIGN.md §10b says how they were chosen.
constexpr double DENOISE_SIGMA_LUMINANCE = 4.0;
constexpr double DENOISE_SIGMA_NORMAL = 64.0;
constexpr double DENOISE_SIGMA_DEPTH = 0.1;

// The call's parameters with the defaults resolved.
struct DenoiseParams {
    double sigma_luminance;
    double sigma_depth;
    uint32_t normal_squarings; // w_n = max(0, n.n')^(2^normal_squarings): the smallest power of two >= sigma_normal, at most 2^10
    uint32_t has_variance;
};
inline DenoiseParams denoise_params(double sigma_luminance, double sigma_normal, double sigma_depth, bool has_variance) {
    DenoiseParams q;
    q.sigma_luminance = sigma_luminance == 0.0 ? DENOISE_SIGMA_LUMINANCE : sigma_luminance;
    q.sigma_depth = sigma_depth == 0.0 ? DENOISE_SIGMA_DEPTH : sigma_depth;
    const double sn = sigma_normal == 0.0 ? DENOISE_SIGMA_NORMAL : sigma_normal;
    q.normal_squarings = 0;
    while (q.normal_squarings < 10u && double(1u << q.normal_squarings) < sn) ++q.normal_squarings;
    q.has_variance = has_variance ? 1u : 0u;
    return q;
}

// One pass's input: row-major, top row first; colour and variance are the demodulated ones.
struct DenoiseView {
    uint32_t width, height;
    const double* colour;   // w*h*3
    const double* variance; // w*h*3, or nullptr
    const double* normal;   // w*h*3
    const double* depth;    // w*h
    const double* alpha;    // w*h
};

RT_HD bool denoise_finite(double v) { return v - v == 0.0; } // false for +-inf and NaN
RT_HD bool denoise_finite3(const double* v) { return denoise_finite(v[0]) && denoise_finite(v[1]) && denoise_finite(v[2]); }
RT_HD double denoise_luminance(const double* c) { // Rec. 709
    return unfused_mul(0.2126, c[0]) + unfused_mul(0.7152, c[1]) + unfused_mul(0.0722, c[2]);
}
// ... and the variance of that sum of independent channels
RT_HD double denoise_luminance_variance(const double* v) {
    return unfused_mul(unfused_mul(0.2126, 0.2126), v[0]) + unfused_mul(unfused_mul(0.7152, 0.7152), v[1]) + unfused_mul(unfused_mul(0.0722, 0.0722), v[2]);
}

// Demodulation of one channel: colour / albedo where the pixel was hit (alpha != 0) and the albedo is large enough to divide by; the
// variance of the pixel mean by albedo^2 likewise.  A pixel with alpha == 0 keeps its value through the whole call, bit for bit.
RT_HD bool denoise_modulated(double albedo, double alpha) { return alpha != 0.0 && albedo > DENOISE_ALBEDO_EPS; }
RT_HD double denoise_demodulate(double colour, double albedo, double alpha) { return denoise_modulated(albedo, alpha) ? colour / albedo : colour; }
RT_HD double denoise_demodulate_variance(double var, double albedo, double alpha) {
    return denoise_modulated(albedo, alpha) ? var / unfused_mul(albedo, albedo) : var;
}
RT_HD double denoise_remodulate(double colour, double albedo, double alpha) { return denoise_modulated(albedo, alpha) ? unfused_mul(colour, albedo) : colour; }
RT_HD double denoise_remodulate_variance(double var, double albedo, double alpha) {
    return denoise_modulated(albedo, alpha) ? unfused_mul(var, unfused_mul(albedo, albedo)) : var;
}

// Gamma + quantise of the output — main.rs:219-225 (`as u8` saturates, NaN -> 0), as rt_core.hpp quantise(double).
RT_HD uint8_t denoise_quantise(double mean) {
    double x = sqrt(mean);
    if (x < 0.0) x = 0.0;
    if (x > 0.999) x = 0.999;
    x = unfused_mul(x, 256.0);
    if (!(x == x) || x <= 0.0) return 0;
    if (x >= 255.0) return 255;
    return uint8_t(x);
}

// ---- The filter itself, stated once for rttnw_denoise and rttnw_reconstruct.  FLAGS is the compile-time switch between the two: with it every
// pixel carries a byte H, "holds a value", beside its colour (`holds`, w*h, row-major; reconstruct.hpp has the why); without it every pixel holds
// a value, `holds` is never read (pass nullptr) and each H below folds to true — what is left is rttnw_denoise's arithmetic, operation for operation.
// The colour and variance of a pixel without H are never read: the tests poison them with NaN.

// Prepare, one channel of one pixel: a pixel with H is demodulated; a pixel without H whose alpha is 0 — every feature sample missed, so
// `albedo` is the background rttnw_render_features stores there, which is also what every render sample of it returns — takes that background
// with variance 0 and holds a value from here on; any other pixel without H keeps H = 0 (its colour and variance are written as 0 and never
// read).  Returns H, the same for the pixel's three channels.  colour / variance: the caller's (variance may be nullptr), not read without H.
template <bool FLAGS>
RT_HD uint8_t atrous_prepare_value(bool holds, const double* colour, const double* variance, double albedo, double alpha, double* out_colour,
                                   double* out_variance) {
    if (!FLAGS || holds) {
        *out_colour = denoise_demodulate(*colour, albedo, alpha);
        if (variance) *out_variance = denoise_demodulate_variance(*variance, albedo, alpha);
        return 1u;
    }
    const bool sky = alpha == 0.0;
    *out_colour = sky ? albedo : 0.0;
    if (variance) *out_variance = 0.0;
    return sky ? 1u : 0u;
}

// Variance of the centre's luminance for the colour stop: the 3x3 neighbourhood's (taps (1, 2, 1) x (1, 2, 1), row-major; taps outside the
// image, with alpha == 0, without H or with a variance that is not finite are dropped), normalised by the weights used.  A per-pixel variance
// from a handful of samples is itself noisy: unsmoothed, a pixel whose few samples happen to agree would refuse every neighbour.
template <bool FLAGS> RT_HD double atrous_centre_variance(const DenoiseView& in, const uint8_t* holds, uint32_t x, uint32_t y) {
    double sum = 0.0, sum_w = 0.0;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = int(x) + dx, yy = int(y) + dy;
            if (xx < 0 || yy < 0 || xx >= int(in.width) || yy >= int(in.height)) continue;
            const size_t q = size_t(yy) * in.width + size_t(xx);
            if (in.alpha[q] == 0.0 || (FLAGS && !holds[q]) || !denoise_finite3(in.variance + q * 3)) continue;
            const double w = double((2 - (dx < 0 ? -dx : dx)) * (2 - (dy < 0 ? -dy : dy)));
            sum = sum + unfused_mul(w, denoise_luminance_variance(in.variance + q * 3));
            sum_w = sum_w + w;
        }
    return sum / sum_w; // (the centre itself is always among the taps: the caller has checked it)
}

// The feature stops of one tap, stated once for the à-trous pass below and the windows of variance.hpp and clamp.hpp: w_n and w_z of the formulas
// below, apart — the pass multiplies its kernel weight in between.  n0, z0, az0 = |z0|: the centre's; n0 and n are three values `step` doubles apart.
struct EdgeStops {
    double wn, wz;
};
RT_HD EdgeStops denoise_edge_stops(const double* n0, double z0, double az0, const double* n, int step, double z, uint32_t normal_squarings,
                                   double sigma_depth) {
    EdgeStops e;
    e.wn = unfused_mul(n0[0], n[0]) + unfused_mul(n0[1], n[step]) + unfused_mul(n0[2], n[2 * step]);
    e.wn = e.wn > 0.0 ? e.wn : 0.0;
    for (uint32_t k = 0; k < normal_squarings; ++k) e.wn = unfused_mul(e.wn, e.wn);
    const double az = z < 0.0 ? -z : z;
    const double qz = (z0 - z) / (unfused_mul(unfused_mul(sigma_depth, az0 + az), 0.5) + DENOISE_TINY);
    const double rz = 1.0 / (1.0 + unfused_mul(qz, qz));
    e.wz = unfused_mul(rz, rz);
    return e;
}

// One pixel of one pass at stride `stride` (2^i in pass i): out_colour[3], out_variance[3] (written only when the view has a variance); returns H'.
//   tap weight  w = h_x h_y * w_n * w_z * w_l,  h = (1, 4, 6, 4, 1) / 16;  taps outside the image, with alpha == 0 or without H are dropped
//   w_n = max(0, n.n')^(2^k)                                             (k squarings)
//   w_z = r^2,  r = 1 / (1 + (dz / (sigma_depth (|z| + |z'|) / 2 + tiny))^2)
//   w_l = 1 / (1 + (dlum / (sigma_luminance sqrt(max(var_lum, 0)) + tiny))^2);  1 without a variance, or where the centre's is not finite
//   colour = sum w c / sum w;  variance = sum w^2 var / (sum w)^2 over the taps whose variance is finite
// A centre with alpha == 0, or whose taps all weigh 0 (a zero normal), passes through, its flag included; so does the variance of a centre whose
// own is not finite.  A centre with H ends with H' = 1.  A centre without H is FILLED from the taps that remain: w = h_x h_y * w_n * w_z (no
// colour stop: it has no colour); with sum w > 0 colour = sum w c / sum w, variance = sum w^2 var / (sum w)^2 over the accepted taps whose
// variance is finite (+inf if none is), H' = 1; otherwise colour 0 and H' = 0.
template <bool FLAGS>
RT_HD uint8_t atrous_filter_pixel(const DenoiseView& in, const uint8_t* holds, const DenoiseParams& prm, uint32_t x, uint32_t y, uint32_t stride,
                                  double* out_colour, double* out_variance) {
    const size_t o = size_t(y) * in.width + x;
    const bool has_var = in.variance != nullptr;
    const bool own = FLAGS ? holds[o] != 0 : true;
    const double* c0 = in.colour + o * 3;
    for (int ch = 0; ch < 3; ++ch) {
        out_colour[ch] = own ? c0[ch] : 0.0;
        if (has_var) out_variance[ch] = own ? in.variance[o * 3 + ch] : 0.0;
    }
    if (in.alpha[o] == 0.0) return own ? 1u : 0u;
    const double* n0 = in.normal + o * 3;
    const double z0 = in.depth[o], az0 = z0 < 0.0 ? -z0 : z0;
    const double lum0 = own ? denoise_luminance(c0) : 0.0;
    const bool var0 = own && has_var && denoise_finite3(in.variance + o * 3);
    double lum_scale = 0.0;
    if (var0) {
        const double vl = atrous_centre_variance<FLAGS>(in, holds, x, y);
        lum_scale = unfused_mul(prm.sigma_luminance, sqrt(vl > 0.0 ? vl : 0.0)) + DENOISE_TINY;
    }
    const bool fill_var = !own && has_var; // a filled centre takes the variance of the taps it was filled from
    bool any_var = false;
    double sum_w = 0.0, sum_c[3] = {0.0, 0.0, 0.0}, sum_v[3] = {0.0, 0.0, 0.0};
    for (int dy = -2; dy <= 2; ++dy)
        for (int dx = -2; dx <= 2; ++dx) {
            const long long xx = (long long)x + (long long)dx * stride, yy = (long long)y + (long long)dy * stride;
            if (xx < 0 || yy < 0 || xx >= (long long)in.width || yy >= (long long)in.height) continue;
            const size_t q = size_t(yy) * in.width + size_t(xx);
            if (in.alpha[q] == 0.0 || (FLAGS && !holds[q])) continue;
            const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
            const double h = double((ax == 0 ? 6 : ax == 1 ? 4 : 1) * (ay == 0 ? 6 : ay == 1 ? 4 : 1)) / 256.0; // exact
            const EdgeStops e = denoise_edge_stops(n0, z0, az0, in.normal + q * 3, 1, in.depth[q], prm.normal_squarings, prm.sigma_depth);
            double wl = 1.0;
            if (var0) {
                const double ql = (lum0 - denoise_luminance(in.colour + q * 3)) / lum_scale;
                wl = 1.0 / (1.0 + unfused_mul(ql, ql));
            }
            const double w = unfused_mul(unfused_mul(unfused_mul(h, e.wn), e.wz), wl);
            sum_w = sum_w + w;
            for (int ch = 0; ch < 3; ++ch) sum_c[ch] = sum_c[ch] + unfused_mul(w, in.colour[q * 3 + ch]);
            if ((var0 || fill_var) && denoise_finite3(in.variance + q * 3)) {
                const double w2 = unfused_mul(w, w);
                for (int ch = 0; ch < 3; ++ch) sum_v[ch] = sum_v[ch] + unfused_mul(w2, in.variance[q * 3 + ch]);
                any_var = true;
            }
        }
    if (!(sum_w > 0.0)) return own ? 1u : 0u;
    const double sw2 = unfused_mul(sum_w, sum_w);
    for (int ch = 0; ch < 3; ++ch) {
        out_colour[ch] = sum_c[ch] / sum_w;
        if (var0) out_variance[ch] = sum_v[ch] / sw2;
        else if (fill_var) out_variance[ch] = any_var ? sum_v[ch] / sw2 : INFINITY;
    }
    return 1u;
}
// rttnw_denoise's pass, by name: what its kernel and tests/denoise_host call
RT_HD void denoise_filter_pixel(const DenoiseView& in, const DenoiseParams& prm, uint32_t x, uint32_t y, uint32_t stride, double* out_colour,
                                double* out_variance) {
    atrous_filter_pixel<false>(in, nullptr, prm, x, y, stride, out_colour, out_variance);
}

// Finish, one pixel: with H the remodulated colour and variance (`remodulate` == false: 0 iterations, the copy), RGBA8 alpha 255; without H
// linear 0, RGBA8 0 0 0 0 and a variance of +inf.  Returns the pixel's out_valid byte.
template <bool FLAGS>
RT_HD uint8_t atrous_finish_pixel(bool holds, bool remodulate, const double* colour, const double* variance, const double* albedo, double alpha,
                                  double* out_colour, uint8_t* out_rgba, double* out_variance) {
    const bool own = !FLAGS || holds;
    for (int ch = 0; ch < 3; ++ch) {
        const double c = !own ? 0.0 : remodulate ? denoise_remodulate(colour[ch], albedo[ch], alpha) : colour[ch];
        out_colour[ch] = c;
        out_rgba[ch] = own ? denoise_quantise(c) : uint8_t(0);
        if (variance) out_variance[ch] = !own ? INFINITY : remodulate ? denoise_remodulate_variance(variance[ch], albedo[ch], alpha) : variance[ch];
    }
    out_rgba[3] = own ? 255 : 0;
    return own ? 1u : 0u;
}

} // namespace rt
