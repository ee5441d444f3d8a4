// svgf.hpp — the arithmetic rttnw_svgf_push and rttnw_svgf_frame add to the stages they compose (include/rttnw_hip.h has the contract, DESIGN.md
// §10b the why), shared by the device kernels (svgf.hip) and the host test harness (tests/svgf_host): the SVGF loop (Schied et al. 2017) over a
// history that stays on the device.  Three per-pixel steps stand here; the estimate between them is variance.hpp's stage B and the filter is
// denoise.hpp's passes, both as they are.
//   ingest      the frame's colour as doubles and, with `demodulate`, divided by the first-hit albedo under rttnw_denoise's rule, with one "was
//               divided" byte per channel
//   accumulate  variance_accumulate_pixel — the reprojection and the four taps computed once — with a third quantity on the same accepted taps:
//               the fed-back colour history H beside the moments M1 and M2.  Each quantity is, bit for bit, what its own entry point computes:
//               M1, M2, length and xy rttnw_temporal_variance's stage A, the colour rttnw_temporal_accumulate's over prev_linear = H
//   emit        the filtered image and the accumulation multiplied back on the channels ingest divided, and the RGBA8
// With rttnw_svgf_set_regress (and the host harness tests/svgf_regress_host) the accumulate step carries two half histories Ha and Hb in H's
// place — svgf_accumulate_halves_pixel, each half rttnw_temporal_accumulate's colour over its own history — and the filter is regress.hpp's over
// the two accumulated halves, as it is.
//
// Everything is double.  + - * /, sqrt, floor and comparisons only, every product through unfused_mul() (adaptive.hpp), the order of every sum
// that of temporal.hpp, so the device code, a g++ host build and a numpy restatement produce the same bits (tests/test_svgf_cpu.py,
// tests/test_gpu_svgf.py).
#pragma once
#include "variance.hpp"
#include "regress.hpp" // rttnw_svgf_set_regress: the regression filter (and, with features == 0, non-local means) as the spatial stage

namespace rt {

// Ingest, one channel of one pixel: the colour the loop accumulates, estimates and filters; `divided`: whether emit multiplies it back
RT_HD double svgf_ingest_value(bool demodulate, double colour, double albedo, double alpha, uint8_t& divided) {
    divided = demodulate && denoise_modulated(albedo, alpha) ? 1u : 0u;
    return divided ? colour / albedo : colour;
}

// Emit, one channel of one pixel
RT_HD double svgf_emit_value(double colour, double albedo, uint8_t divided) { return divided ? unfused_mul(colour, albedo) : colour; }

struct SvgfAccumulated {
    double m1[3], m2[3], a[3], length, xy[2]; // a: the filter's input — the blend over H with `feedback`, m1 without
};

// Accumulate, one pixel: variance_accumulate_pixel's expressions in its order, and with `feedback` (a fed-back history exists: prev_history is
// read) temporal_pixel's colour over prev_history on the same taps.  The `prev_*` arrays are not read without a history.
RT_HD SvgfAccumulated svgf_accumulate_pixel(uint32_t w, uint32_t h, uint32_t x, uint32_t y, const TemporalParams& q, bool feedback, const double* linear,
                                            const double* normal, const double* depth, const double* alpha, const double* prev_moment1,
                                            const double* prev_moment2, const double* prev_history, const double* prev_length, const double* prev_normal,
                                            const double* prev_depth, const double* prev_alpha) {
    const size_t p = size_t(y) * w + x, o = p * 3;
    const double nan = NAN;
    SvgfAccumulated out;
    double sq[3];
    for (int ch = 0; ch < 3; ++ch) { // this frame alone: no history, a miss, a reset
        out.m1[ch] = out.a[ch] = linear[o + ch];
        out.m2[ch] = sq[ch] = unfused_mul(linear[o + ch], linear[o + ch]);
    }
    out.length = 1.0;
    out.xy[0] = out.xy[1] = nan;
    const double al = alpha[p];
    if (!q.has_history || al == 0.0) return out;
    double fx, fy, zq;
    if (!temporal_where(w, h, x, y, q, depth[p] / al, fx, fy, zq)) return out;
    out.xy[0] = fx;
    out.xy[1] = fy;
    const double x0 = floor(fx), y0 = floor(fy);
    const double ax = fx - x0, ay = fy - y0;
    const int ix = int(x0), iy = int(y0); // -1 .. w - 1, -1 .. h - 1
    const double nn = temporal_dot(normal + o, normal + o);
    double sw = 0.0, sl = 0.0, s1[3] = {0.0, 0.0, 0.0}, s2[3] = {0.0, 0.0, 0.0}, sh[3] = {0.0, 0.0, 0.0};
    for (int j = 0; j < 2; ++j)
        for (int i = 0; i < 2; ++i) { // 00, 10, 01, 11
            const int tx = ix + i, ty = iy + j;
            if (tx < 0 || tx >= int(w) || ty < 0 || ty >= int(h)) continue;
            const size_t tp = size_t(ty) * w + size_t(tx);
            if (!temporal_accepts(q, tp, normal + o, nn, zq, prev_length, prev_normal, prev_depth, prev_alpha)) continue;
            const double wt = unfused_mul(i ? ax : 1.0 - ax, j ? ay : 1.0 - ay);
            sw = sw + wt;
            sl = sl + unfused_mul(wt, prev_length[tp]);
            for (int ch = 0; ch < 3; ++ch) {
                s1[ch] = s1[ch] + unfused_mul(wt, prev_moment1[tp * 3 + ch]);
                s2[ch] = s2[ch] + unfused_mul(wt, prev_moment2[tp * 3 + ch]);
                if (feedback) sh[ch] = sh[ch] + unfused_mul(wt, prev_history[tp * 3 + ch]);
            }
        }
    if (!(sw > 0.0)) return out; // reset
    const double grown = sl / sw + 1.0;
    const double n = grown < q.max_history ? grown : q.max_history;
    const double wa = 1.0 / n, wb = 1.0 - wa;
    for (int ch = 0; ch < 3; ++ch) {
        out.m1[ch] = unfused_mul(wb, s1[ch] / sw) + unfused_mul(wa, linear[o + ch]);
        out.m2[ch] = unfused_mul(wb, s2[ch] / sw) + unfused_mul(wa, sq[ch]);
        out.a[ch] = feedback ? unfused_mul(wb, sh[ch] / sw) + unfused_mul(wa, linear[o + ch]) : out.m1[ch];
    }
    out.length = n;
    return out;
}

struct SvgfAccumulatedHalves {
    double m1[3], m2[3], a[3], b[3], length, xy[2]; // a, b: the two accumulated halves Aa and Ab, the regression stage's inputs
};

// Accumulate with rttnw_svgf_set_regress, one pixel: svgf_accumulate_pixel's expressions in its order, and the two half histories Ha and Hb on the
// accepted taps where H rides there — each blended with its own half of the frame, temporal_pixel's colour over prev_half_a / prev_half_b.  M1, M2,
// length and xy are svgf_accumulate_pixel's of `linear` bit for bit.  Every pass-through case leaves a half as the frame's.  The `prev_*` arrays
// are not read without a history.
RT_HD SvgfAccumulatedHalves svgf_accumulate_halves_pixel(uint32_t w, uint32_t h, uint32_t x, uint32_t y, const TemporalParams& q, const double* linear,
                                                        const double* half_a, const double* half_b, const double* normal, const double* depth,
                                                        const double* alpha, const double* prev_moment1, const double* prev_moment2,
                                                        const double* prev_half_a, const double* prev_half_b, const double* prev_length,
                                                        const double* prev_normal, const double* prev_depth, const double* prev_alpha) {
    const size_t p = size_t(y) * w + x, o = p * 3;
    const double nan = NAN;
    SvgfAccumulatedHalves out;
    double sq[3];
    for (int ch = 0; ch < 3; ++ch) { // this frame alone: no history, a miss, a reset
        out.m1[ch] = linear[o + ch];
        out.m2[ch] = sq[ch] = unfused_mul(linear[o + ch], linear[o + ch]);
        out.a[ch] = half_a[o + ch];
        out.b[ch] = half_b[o + ch];
    }
    out.length = 1.0;
    out.xy[0] = out.xy[1] = nan;
    const double al = alpha[p];
    if (!q.has_history || al == 0.0) return out;
    double fx, fy, zq;
    if (!temporal_where(w, h, x, y, q, depth[p] / al, fx, fy, zq)) return out;
    out.xy[0] = fx;
    out.xy[1] = fy;
    const double x0 = floor(fx), y0 = floor(fy);
    const double ax = fx - x0, ay = fy - y0;
    const int ix = int(x0), iy = int(y0); // -1 .. w - 1, -1 .. h - 1
    const double nn = temporal_dot(normal + o, normal + o);
    double sw = 0.0, sl = 0.0, s1[3] = {0.0, 0.0, 0.0}, s2[3] = {0.0, 0.0, 0.0}, sa[3] = {0.0, 0.0, 0.0}, sb[3] = {0.0, 0.0, 0.0};
    for (int j = 0; j < 2; ++j)
        for (int i = 0; i < 2; ++i) { // 00, 10, 01, 11
            const int tx = ix + i, ty = iy + j;
            if (tx < 0 || tx >= int(w) || ty < 0 || ty >= int(h)) continue;
            const size_t tp = size_t(ty) * w + size_t(tx);
            if (!temporal_accepts(q, tp, normal + o, nn, zq, prev_length, prev_normal, prev_depth, prev_alpha)) continue;
            const double wt = unfused_mul(i ? ax : 1.0 - ax, j ? ay : 1.0 - ay);
            sw = sw + wt;
            sl = sl + unfused_mul(wt, prev_length[tp]);
            for (int ch = 0; ch < 3; ++ch) {
                s1[ch] = s1[ch] + unfused_mul(wt, prev_moment1[tp * 3 + ch]);
                s2[ch] = s2[ch] + unfused_mul(wt, prev_moment2[tp * 3 + ch]);
                sa[ch] = sa[ch] + unfused_mul(wt, prev_half_a[tp * 3 + ch]);
                sb[ch] = sb[ch] + unfused_mul(wt, prev_half_b[tp * 3 + ch]);
            }
        }
    if (!(sw > 0.0)) return out; // reset
    const double grown = sl / sw + 1.0;
    const double n = grown < q.max_history ? grown : q.max_history;
    const double wa = 1.0 / n, wb = 1.0 - wa;
    for (int ch = 0; ch < 3; ++ch) {
        out.m1[ch] = unfused_mul(wb, s1[ch] / sw) + unfused_mul(wa, linear[o + ch]);
        out.m2[ch] = unfused_mul(wb, s2[ch] / sw) + unfused_mul(wa, sq[ch]);
        out.a[ch] = unfused_mul(wb, sa[ch] / sw) + unfused_mul(wa, half_a[o + ch]);
        out.b[ch] = unfused_mul(wb, sb[ch] / sw) + unfused_mul(wa, half_b[o + ch]);
    }
    out.length = n;
    return out;
}

// The mean of the two accumulated halves, one channel: accumulated_rgb before emit multiplies it back ((Aa + Ab) * 0.5, nlm.hpp's mean)
RT_HD double svgf_halves_mean(double a, double b) { return nlm_mean(a, b); }

// The variance handed to the regression stage with variance_source 0: each half is a mean over half the samples of M1, so twice M1's — one sum
RT_HD double svgf_half_variance(double var) { return var + var; }

// The device's blocks (svgf.hip): the accumulate kernel's are variance.hip's, 64 pixels of a row by 4 rows
constexpr uint32_t SVGF_BLOCK_X = VARIANCE_BLOCK_X, SVGF_BLOCK_Y = VARIANCE_BLOCK_Y;

} // namespace rt
