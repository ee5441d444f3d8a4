// probe.hpp — the arithmetic of rttnw_temporal_probe (include/rttnw_hip.h has the contract, DESIGN.md §10b the why), shared by the device kernel
// (probe.hip) and the host test harness (tests/probe_host): where each pixel's history is and how long, from the frame's first-hit features and the
// state's alone — no colour — and from that length how many times the frame's samples the pixel is given.  The geometry and the acceptance are
// temporal.hpp's own functions (temporal_where, temporal_accepts), called in temporal_pixel's order; nothing of them is restated here.
//
// Everything is double.  + - * /, sqrt, floor and comparisons only, every product through unfused_mul() (adaptive.hpp), the order of every sum
// fixed here, so the device code, a g++ host build and a numpy restatement produce the same bits (tests/test_probe_cpu.py, tests/test_gpu_probe.py):
//   taps 00, 10, 01, 11 as temporal_pixel takes them: wt = (i ? ax : 1 - ax) * (j ? ay : 1 - ay);  sw = sw + wt;  sl = sl + wt * prev_length[tp]
//   Lp = sw > 0 ? sl / sw : 0          (0 as well without a history, on a miss, and where the pixel has no place in the previous frame)
//   k = floor(fill / (Lp + 1));  m = the largest of 1, 2, 4, 8 that is <= min(k, boost);  m = 1 where k < 1 (or NaN) and where alpha == 0
#pragma once
#include "temporal.hpp"

namespace rt {

// The library defaults (a 0 in rttnw_sampling_params)
constexpr uint32_t SAMPLING_BOOST = 8;
constexpr double SAMPLING_FILL = 8.0;

// rttnw_sampling_params with the defaults resolved
struct SamplingParams {
    double fill;
    uint32_t boost; // 1, 2, 4 or 8
};

inline SamplingParams sampling_params(uint32_t boost, double fill) {
    SamplingParams a;
    a.fill = fill == 0.0 ? SAMPLING_FILL : fill;
    a.boost = boost == 0u ? SAMPLING_BOOST : boost;
    return a;
}

// The multiplier of a pixel whose reprojected history counts `length` frames; `hit`: this frame's alpha != 0.  Every comparison with a NaN is
// false, so a NaN length gets 1.
RT_HD uint32_t probe_multiplier(const SamplingParams& a, double length, bool hit) {
    if (!hit) return 1u;
    const double k = floor(a.fill / (length + 1.0));
    uint32_t m = 1u;
    if (k >= 2.0 && a.boost >= 2u) m = 2u;
    if (k >= 4.0 && a.boost >= 4u) m = 4u;
    if (k >= 8.0 && a.boost >= 8u) m = 8u;
    return m;
}

struct ProbePixel {
    double length, xy[2];
    uint32_t multiplier;
};

// One pixel of the call: temporal_pixel's control flow without the colour.  `prev_*` are not read without a history.
RT_HD ProbePixel probe_pixel(uint32_t w, uint32_t h, uint32_t x, uint32_t y, const TemporalParams& q, const SamplingParams& a, const double* normal,
                             const double* depth, const double* alpha, const double* prev_length, const double* prev_normal, const double* prev_depth,
                             const double* prev_alpha) {
    const size_t p = size_t(y) * w + x, o = p * 3;
    const double nan = NAN;
    ProbePixel out;
    out.length = 0.0; // no history, a miss, a reset
    out.xy[0] = out.xy[1] = nan;
    const double al = alpha[p];
    out.multiplier = probe_multiplier(a, 0.0, al != 0.0);
    if (!q.has_history || al == 0.0) return out;
    double fx, fy, zq;
    if (!temporal_where(w, h, x, y, q, depth[p] / al, fx, fy, zq)) return out;
    out.xy[0] = fx;
    out.xy[1] = fy;
    const double x0 = floor(fx), y0 = floor(fy);
    const double ax = fx - x0, ay = fy - y0;
    const int ix = int(x0), iy = int(y0); // -1 .. w - 1, -1 .. h - 1
    const double nn = temporal_dot(normal + o, normal + o);
    double sw = 0.0, sl = 0.0;
    for (int j = 0; j < 2; ++j)
        for (int i = 0; i < 2; ++i) { // 00, 10, 01, 11
            const int tx = ix + i, ty = iy + j;
            if (tx < 0 || tx >= int(w) || ty < 0 || ty >= int(h)) continue;
            const size_t tp = size_t(ty) * w + size_t(tx);
            if (!temporal_accepts(q, tp, normal + o, nn, zq, prev_length, prev_normal, prev_depth, prev_alpha)) continue;
            const double wt = unfused_mul(i ? ax : 1.0 - ax, j ? ay : 1.0 - ay);
            sw = sw + wt;
            sl = sl + unfused_mul(wt, prev_length[tp]);
        }
    if (!(sw > 0.0)) return out; // reset
    out.length = sl / sw;
    out.multiplier = probe_multiplier(a, out.length, true);
    return out;
}

} // namespace rt
