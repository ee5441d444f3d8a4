// reconstruct.hpp — the arithmetic of rttnw_reconstruct (include/rttnw_hip.h has the contract, DESIGN.md §10b the why), shared by the device
// kernels (reconstruct.hip) and the host test harness (tests/reconstruct_host): rttnw_denoise's à-trous filter over an image of which only
// some pixels hold a value.  Every pixel carries a flag H, "holds a value", through the passes beside its colour: a tap without H is dropped
// like a tap outside the image, and a centre without H is FILLED from the taps that remain — weighted by the features alone, it has no colour
// to compare — and holds a value from then on.  Pass i reaches 2 * 2^i pixels to either side, so a lattice of spacing 2^L is filled after
// L passes at the latest where the features let neighbours through.
//
// denoise.hpp's helpers are reused and denoise_filter_pixel itself is left alone (rttnw_denoise's bits cannot move); with every flag set,
// reconstruct_filter_pixel performs denoise_filter_pixel's operations in its order, so the two agree bit for bit (tests/test_reconstruct_cpu.py).
// The colour and variance of a pixel without H are never read: the tests poison them with NaN.
#pragma once
#include "denoise.hpp"

namespace rt {

// One pass's input: denoise.hpp's view and the flags, a byte per pixel, row-major.
struct ReconstructView {
    DenoiseView img;
    const uint8_t* holds; // w*h, nonzero = the pixel holds a value
};

// Prepare, one pixel: a pixel with H is demodulated as in rttnw_denoise; a pixel without H whose alpha is 0 — every feature sample missed,
// so `albedo` is the background rttnw_render_features stores there, which is also what every render sample of it returns — takes that
// background with variance 0 and holds a value from here on; any other pixel without H keeps H = 0 (its colour and variance are written as 0
// and never read).  Returns H.  colour / variance: the caller's pixel (3 doubles each, variance may be nullptr), not read without H.
RT_HD uint8_t reconstruct_prepare_pixel(bool holds, const double* colour, const double* variance, const double* albedo, double alpha,
                                        double* out_colour, double* out_variance) {
    if (holds) {
        for (int ch = 0; ch < 3; ++ch) {
            out_colour[ch] = denoise_demodulate(colour[ch], albedo[ch], alpha);
            if (variance) out_variance[ch] = denoise_demodulate_variance(variance[ch], albedo[ch], alpha);
        }
        return 1u;
    }
    const bool sky = alpha == 0.0;
    for (int ch = 0; ch < 3; ++ch) {
        out_colour[ch] = sky ? albedo[ch] : 0.0;
        if (variance) out_variance[ch] = 0.0;
    }
    return sky ? 1u : 0u;
}

// denoise_centre_variance over the taps that hold a value (the centre itself is among them: the caller has checked it)
RT_HD double reconstruct_centre_variance(const ReconstructView& rv, uint32_t x, uint32_t y) {
    const DenoiseView& in = rv.img;
    double sum = 0.0, sum_w = 0.0;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = int(x) + dx, yy = int(y) + dy;
            if (xx < 0 || yy < 0 || xx >= int(in.width) || yy >= int(in.height)) continue;
            const size_t q = size_t(yy) * in.width + size_t(xx);
            if (in.alpha[q] == 0.0 || !rv.holds[q] || !denoise_finite3(in.variance + q * 3)) continue;
            const double w = double((2 - (dx < 0 ? -dx : dx)) * (2 - (dy < 0 ? -dy : dy)));
            sum = sum + unfused_mul(w, denoise_luminance_variance(in.variance + q * 3));
            sum_w = sum_w + w;
        }
    return sum / sum_w;
}

// One pixel of one pass at stride `stride`: out_colour[3], out_variance[3] (written only when the view has a variance); returns H'.
//   a tap is dropped when it lies outside the image, has alpha == 0 or has H == 0
//   a centre with alpha == 0 passes through, its flag included
//   a centre with H: denoise_filter_pixel on the remaining taps (the 3x3 of its colour stop likewise drops taps without H); H' = 1
//   a centre without H: w = h_x h_y * w_n * w_z (no colour stop: it has no colour); with sum w > 0 colour = sum w c / sum w, variance =
//     sum w^2 var / (sum w)^2 over the accepted taps whose variance is finite (+inf if none is), H' = 1; otherwise colour 0 and H' = 0
RT_HD uint8_t reconstruct_filter_pixel(const ReconstructView& rv, const DenoiseParams& prm, uint32_t x, uint32_t y, uint32_t stride,
                                       double* out_colour, double* out_variance) {
    const DenoiseView& in = rv.img;
    const size_t o = size_t(y) * in.width + x;
    const bool has_var = in.variance != nullptr;
    const bool own = rv.holds[o] != 0;
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
        const double vl = reconstruct_centre_variance(rv, x, y);
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
            if (in.alpha[q] == 0.0 || !rv.holds[q]) continue;
            const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
            const double h = double((ax == 0 ? 6 : ax == 1 ? 4 : 1) * (ay == 0 ? 6 : ay == 1 ? 4 : 1)) / 256.0; // exact
            const double* n = in.normal + q * 3;
            double wn = unfused_mul(n0[0], n[0]) + unfused_mul(n0[1], n[1]) + unfused_mul(n0[2], n[2]);
            wn = wn > 0.0 ? wn : 0.0;
            for (uint32_t k = 0; k < prm.normal_squarings; ++k) wn = unfused_mul(wn, wn);
            const double z = in.depth[q], az = z < 0.0 ? -z : z;
            const double qz = (z0 - z) / (unfused_mul(unfused_mul(prm.sigma_depth, az0 + az), 0.5) + DENOISE_TINY);
            const double rz = 1.0 / (1.0 + unfused_mul(qz, qz));
            const double wz = unfused_mul(rz, rz);
            double wl = 1.0;
            if (var0) {
                const double ql = (lum0 - denoise_luminance(in.colour + q * 3)) / lum_scale;
                wl = 1.0 / (1.0 + unfused_mul(ql, ql));
            }
            const double w = unfused_mul(unfused_mul(unfused_mul(h, wn), wz), wl);
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

// Finish, one pixel: with H the remodulated colour and variance (`remodulate` == false: 0 iterations, the copy), RGBA8 alpha 255; without H
// linear 0, RGBA8 0 0 0 0 and a variance of +inf.  Returns the pixel's out_valid byte.
RT_HD uint8_t reconstruct_finish_pixel(bool holds, bool remodulate, const double* colour, const double* variance, const double* albedo, double alpha,
                                       double* out_colour, uint8_t* out_rgba, double* out_variance) {
    for (int ch = 0; ch < 3; ++ch) {
        double c = 0.0, v = INFINITY;
        if (holds) {
            c = remodulate ? denoise_remodulate(colour[ch], albedo[ch], alpha) : colour[ch];
            if (variance) v = remodulate ? denoise_remodulate_variance(variance[ch], albedo[ch], alpha) : variance[ch];
        }
        out_colour[ch] = c;
        out_rgba[ch] = holds ? denoise_quantise(c) : uint8_t(0);
        if (variance) out_variance[ch] = v;
    }
    out_rgba[3] = holds ? 255 : 0;
    return holds ? 1u : 0u;
}

} // namespace rt
