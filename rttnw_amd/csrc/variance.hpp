// variance.hpp — the arithmetic of rttnw_temporal_variance (include/rttnw_hip.h has the contract, DESIGN.md §10b the why), shared by the device
// kernels (variance.hip) and the host test harness (tests/variance_host): the variance estimation of SVGF (Schied et al. 2017, §4.2) behind the
// accumulation of temporal.hpp.  Stage A is rttnw_temporal_accumulate without variances — its reprojection, taps and blend, through temporal_taps,
// temporal_tap_sum and temporal_blend — with the second moment riding on the accepted taps.  Stage B reads stage A's outputs: where a pixel's
// history is long enough the variance of its mean comes from the two moments, elsewhere from a window guided by normal and depth.
//
// Everything is double.  + - * /, sqrt, floor and comparisons only, every product through unfused_mul() (adaptive.hpp), the order of every sum
// fixed here, so the device code, a g++ host build and a numpy restatement produce the same bits (tests/test_variance_cpu.py,
// tests/test_gpu_variance.py):
//   A: h2 = (sum wt m2') / W;  s = cur * cur;  out_m2 = (1 - a) * h2 + a * s;  out_m2 = s wherever the colour passes through
//   B: pos(x) = x < 0 ? 0 : x;  alpha == 0: 0;  N >= min_temporal: pos(m2 - m1 m1) / (N - 1);  otherwise over the window, dy outer, dx inner,
//      w = w_n w_z (denoise.hpp, denoise_edge_stops), Sw = sum w, M1 = (sum w m1') / Sw, M2 = (sum w m2') / Sw:  pos(M2 - M1 M1) / N;
//      Sw > 0 false: pos(m2 - m1 m1) / N
#pragma once
#include "temporal.hpp"

namespace rt {

constexpr uint32_t VARIANCE_MAX_RADIUS = 4;
// The library defaults (a 0 in rttnw_variance_params)
constexpr uint32_t VARIANCE_MIN_TEMPORAL = 4, VARIANCE_RADIUS = 3;

// Stage B's parameters with the defaults resolved
struct VarianceParams {
    double min_temporal, sigma_depth;
    uint32_t radius, normal_squarings; // normal_squarings: as DenoiseParams
};
inline VarianceParams variance_params(uint32_t min_temporal, uint32_t radius, double sigma_normal, double sigma_depth) {
    const DenoiseParams d = denoise_params(0.0, sigma_normal, sigma_depth, false);
    VarianceParams q;
    q.min_temporal = double(min_temporal == 0 ? VARIANCE_MIN_TEMPORAL : min_temporal);
    q.sigma_depth = d.sigma_depth;
    q.radius = radius == 0 ? VARIANCE_RADIUS : radius;
    q.normal_squarings = d.normal_squarings;
    return q;
}

struct VarianceAccumulated {
    double c[3], m2[3], length, xy[2];
};

// Stage A on taps that are already taken (svgf.hpp takes them once for more quantities): `cur` is this pixel's colour; every pass-through case
// leaves the colour and its square.
RT_HD VarianceAccumulated variance_accumulate_taps(const TemporalTaps& t, const TemporalParams& q, const double* cur, const double* prev_linear,
                                                   const double* prev_moment2) {
    VarianceAccumulated out;
    double sq[3];
    for (int ch = 0; ch < 3; ++ch) { // this frame alone: no history, a miss, a reset
        out.c[ch] = cur[ch];
        out.m2[ch] = sq[ch] = unfused_mul(cur[ch], cur[ch]);
    }
    out.length = 1.0;
    out.xy[0] = t.xy[0];
    out.xy[1] = t.xy[1];
    if (!t.blend) return out;
    double sc[3], s2[3];
    temporal_tap_sum(t, prev_linear, sc);
    temporal_tap_sum(t, prev_moment2, s2);
    const TemporalBlend b = temporal_blend(t, q);
    for (int ch = 0; ch < 3; ++ch) {
        out.c[ch] = unfused_mul(b.wb, sc[ch] / t.sw) + unfused_mul(b.wa, cur[ch]);
        out.m2[ch] = unfused_mul(b.wb, s2[ch] / t.sw) + unfused_mul(b.wa, sq[ch]);
    }
    out.length = b.n;
    return out;
}

// Stage A, one pixel: temporal.hpp's taps — so c, length and xy are temporal_pixel's bits without variances — and the second moment beside the
// colour.  The `prev_*` arrays are not read without a history.
RT_HD VarianceAccumulated variance_accumulate_pixel(uint32_t w, uint32_t h, uint32_t x, uint32_t y, const TemporalParams& q, const double* linear,
                                                    const double* normal, const double* depth, const double* alpha, const double* prev_linear,
                                                    const double* prev_moment2, const double* prev_length, const double* prev_normal,
                                                    const double* prev_depth, const double* prev_alpha) {
    const TemporalTaps t = temporal_taps(w, h, x, y, q, normal, depth, alpha, prev_length, prev_normal, prev_depth, prev_alpha);
    return variance_accumulate_taps(t, q, linear + (size_t(y) * w + x) * 3, prev_linear, prev_moment2);
}

// What stage B reads, as a window onto the image: element (0, 0) of the view is image pixel (x0, y0), rows are `stride` pixels apart; channel ch
// of a three-channel quantity of view pixel q is at [q * pixel_step + ch * channel_step].  The whole image in global memory: x0 = y0 = 0,
// stride = width, steps 3 and 1.  The device's tile in LDS (variance.hip): planes, steps 1 and the plane's size.
struct VarianceView {
    const double *alpha, *depth, *normal, *m1, *m2;
    int x0, y0, stride, pixel_step, channel_step;
};
RT_HD int variance_at(const VarianceView& v, int x, int y) { return (y - v.y0) * v.stride + (x - v.x0); }

RT_HD double variance_pos(double v) { return v < 0.0 ? 0.0 : v; } // a NaN stays a NaN

// Stage B, one pixel (x, y) of a w x h image with alpha != 0 and a history shorter than min_temporal: the spatial estimate over the window
RT_HD void variance_spatial(const VarianceView& v, const VarianceParams& prm, int w, int h, int x, int y, double n_frames, double* out) {
    const int c = variance_at(v, x, y);
    double n0[3], m10[3], m20[3];
    for (int ch = 0; ch < 3; ++ch) {
        n0[ch] = v.normal[c * v.pixel_step + ch * v.channel_step];
        m10[ch] = v.m1[c * v.pixel_step + ch * v.channel_step];
        m20[ch] = v.m2[c * v.pixel_step + ch * v.channel_step];
    }
    const double z0 = v.depth[c], az0 = z0 < 0.0 ? -z0 : z0;
    const int radius = int(prm.radius);
    double sw = 0.0, s1[3] = {0.0, 0.0, 0.0}, s2[3] = {0.0, 0.0, 0.0};
    for (int dy = -radius; dy <= radius; ++dy)
        for (int dx = -radius; dx <= radius; ++dx) {
            const int xx = x + dx, yy = y + dy;
            if (xx < 0 || yy < 0 || xx >= w || yy >= h) continue;
            const int q = variance_at(v, xx, yy);
            if (v.alpha[q] == 0.0) continue;
            const int q3 = q * v.pixel_step;
            const EdgeStops e = denoise_edge_stops(n0, z0, az0, v.normal + q3, v.channel_step, v.depth[q], prm.normal_squarings, prm.sigma_depth);
            const double wt = unfused_mul(e.wn, e.wz);
            sw = sw + wt;
            for (int ch = 0; ch < 3; ++ch) {
                s1[ch] = s1[ch] + unfused_mul(wt, v.m1[q3 + ch * v.channel_step]);
                s2[ch] = s2[ch] + unfused_mul(wt, v.m2[q3 + ch * v.channel_step]);
            }
        }
    const bool any = sw > 0.0;
    for (int ch = 0; ch < 3; ++ch) {
        const double a1 = any ? s1[ch] / sw : m10[ch], a2 = any ? s2[ch] / sw : m20[ch];
        out[ch] = variance_pos(a2 - unfused_mul(a1, a1)) / n_frames;
    }
}

// Whether stage B takes the window at a pixel: it was hit and its history is too short to trust
RT_HD bool variance_is_spatial(const VarianceParams& prm, double alpha, double n_frames) { return alpha != 0.0 && !(n_frames >= prm.min_temporal); }

// Stage B's two other branches, one pixel: the background is exact; a long history gives the unbiased variance of the mean of its N frames
RT_HD void variance_temporal(double alpha, double n_frames, const double* m1, const double* m2, double* out) {
    for (int ch = 0; ch < 3; ++ch) out[ch] = alpha == 0.0 ? 0.0 : variance_pos(m2[ch] - unfused_mul(m1[ch], m1[ch])) / (n_frames - 1.0);
}

// Stage B, one pixel, over the whole image in global memory: what the host harness runs
RT_HD void variance_estimate_pixel(uint32_t w, uint32_t h, uint32_t x, uint32_t y, const VarianceParams& prm, const double* m1, const double* m2,
                                   const double* length, const double* normal, const double* depth, const double* alpha, double* out) {
    const size_t p = size_t(y) * w + x;
    if (variance_is_spatial(prm, alpha[p], length[p])) {
        const VarianceView v = {alpha, depth, normal, m1, m2, 0, 0, int(w), 3, 1};
        variance_spatial(v, prm, int(w), int(h), int(x), int(y), length[p], out);
    } else {
        variance_temporal(alpha[p], length[p], m1 + p * 3, m2 + p * 3, out);
    }
}

// The device's blocks (variance.hip): temporal.hip's, 64 pixels of a row by 4 rows; stage B's tile in LDS is the block and a halo of the radius,
// eleven planes of doubles (alpha, depth, normal, m1, m2)
constexpr uint32_t VARIANCE_BLOCK_X = TEMPORAL_BLOCK_X, VARIANCE_BLOCK_Y = TEMPORAL_BLOCK_Y, VARIANCE_PLANES = 11;
constexpr size_t variance_lds_bytes(uint32_t radius) {
    return size_t(VARIANCE_BLOCK_X + 2 * radius) * (VARIANCE_BLOCK_Y + 2 * radius) * VARIANCE_PLANES * sizeof(double);
}

} // namespace rt
