// svgf.hpp — the arithmetic rttnw_svgf_push and rttnw_svgf_frame add to the stages they compose (include/rttnw_hip.h has the contract, DESIGN.md
// §10b the why), shared by the device kernels (svgf.hip) and the host test harness (tests/svgf_host): the SVGF loop (Schied et al. 2017) over a
// history that stays on the device.  Three per-pixel steps stand here; the estimate between them is variance.hpp's stage B and the filter is
// denoise.hpp's passes, both as they are.
//   ingest      the frame's colour as doubles and, with `demodulate`, divided by the first-hit albedo under rttnw_denoise's rule, with one "was
//               divided" byte per channel
//   accumulate  variance.hpp's stage A on temporal.hpp's taps — the reprojection and the four taps computed once — with a third quantity on them:
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

// Accumulate, one pixel: temporal.hpp's taps once, variance.hpp's stage A on them over prev_moment1 and prev_moment2, and with `feedback` (a
// fed-back history exists: prev_history is read) temporal_pixel's colour over prev_history on the same taps.  The `prev_*` arrays are not read
// without a history.
RT_HD SvgfAccumulated svgf_accumulate_pixel(uint32_t w, uint32_t h, uint32_t x, uint32_t y, const TemporalParams& q, bool feedback, const double* linear,
                                            const double* normal, const double* depth, const double* alpha, const double* prev_moment1,
                                            const double* prev_moment2, const double* prev_history, const double* prev_length, const double* prev_normal,
                                            const double* prev_depth, const double* prev_alpha) {
    const size_t o = (size_t(y) * w + x) * 3;
    const TemporalTaps t = temporal_taps(w, h, x, y, q, normal, depth, alpha, prev_length, prev_normal, prev_depth, prev_alpha);
    const VarianceAccumulated m = variance_accumulate_taps(t, q, linear + o, prev_moment1, prev_moment2);
    SvgfAccumulated out;
    for (int ch = 0; ch < 3; ++ch) {
        out.m1[ch] = out.a[ch] = m.c[ch];
        out.m2[ch] = m.m2[ch];
    }
    out.length = m.length;
    out.xy[0] = m.xy[0];
    out.xy[1] = m.xy[1];
    if (!feedback || !t.blend) return out;
    double sh[3];
    temporal_tap_sum(t, prev_history, sh);
    const TemporalBlend b = temporal_blend(t, q);
    for (int ch = 0; ch < 3; ++ch) out.a[ch] = unfused_mul(b.wb, sh[ch] / t.sw) + unfused_mul(b.wa, linear[o + ch]);
    return out;
}

struct SvgfAccumulatedHalves {
    double m1[3], m2[3], a[3], b[3], length, xy[2]; // a, b: the two accumulated halves Aa and Ab, the regression stage's inputs
};

// Accumulate with rttnw_svgf_set_regress, one pixel: svgf_accumulate_pixel's M1, M2, length and xy of `linear`, and the two half histories Ha and Hb
// on the same taps where H rides there — each blended with its own half of the frame, temporal_pixel's colour over prev_half_a / prev_half_b.  Every
// pass-through case leaves a half as the frame's.  The `prev_*` arrays are not read without a history.
RT_HD SvgfAccumulatedHalves svgf_accumulate_halves_pixel(uint32_t w, uint32_t h, uint32_t x, uint32_t y, const TemporalParams& q, const double* linear,
                                                        const double* half_a, const double* half_b, const double* normal, const double* depth,
                                                        const double* alpha, const double* prev_moment1, const double* prev_moment2,
                                                        const double* prev_half_a, const double* prev_half_b, const double* prev_length,
                                                        const double* prev_normal, const double* prev_depth, const double* prev_alpha) {
    const size_t o = (size_t(y) * w + x) * 3;
    const TemporalTaps t = temporal_taps(w, h, x, y, q, normal, depth, alpha, prev_length, prev_normal, prev_depth, prev_alpha);
    const VarianceAccumulated m = variance_accumulate_taps(t, q, linear + o, prev_moment1, prev_moment2);
    SvgfAccumulatedHalves out;
    for (int ch = 0; ch < 3; ++ch) {
        out.m1[ch] = m.c[ch];
        out.m2[ch] = m.m2[ch];
        out.a[ch] = half_a[o + ch];
        out.b[ch] = half_b[o + ch];
    }
    out.length = m.length;
    out.xy[0] = m.xy[0];
    out.xy[1] = m.xy[1];
    if (!t.blend) return out;
    double sa[3], sb[3];
    temporal_tap_sum(t, prev_half_a, sa);
    temporal_tap_sum(t, prev_half_b, sb);
    const TemporalBlend b = temporal_blend(t, q);
    for (int ch = 0; ch < 3; ++ch) {
        out.a[ch] = unfused_mul(b.wb, sa[ch] / t.sw) + unfused_mul(b.wa, half_a[o + ch]);
        out.b[ch] = unfused_mul(b.wb, sb[ch] / t.sw) + unfused_mul(b.wa, half_b[o + ch]);
    }
    return out;
}

// The mean of the two accumulated halves, one channel: accumulated_rgb before emit multiplies it back ((Aa + Ab) * 0.5, nlm.hpp's mean)
RT_HD double svgf_halves_mean(double a, double b) { return nlm_mean(a, b); }

// The variance handed to the regression stage with variance_source 0: each half is a mean over half the samples of M1, so twice M1's — one sum
RT_HD double svgf_half_variance(double var) { return var + var; }

// The device's blocks (svgf.hip): the accumulate kernel's are variance.hip's, 64 pixels of a row by 4 rows
constexpr uint32_t SVGF_BLOCK_X = VARIANCE_BLOCK_X, SVGF_BLOCK_Y = VARIANCE_BLOCK_Y;

} // namespace rt
