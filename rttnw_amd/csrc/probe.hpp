// probe.hpp — the arithmetic of rttnw_temporal_probe (include/rttnw_hip.h has the contract, DESIGN.md §10b the why), shared by the device kernel
// (probe.hip) and the host test harness (tests/probe_host): where each pixel's history is and how long, from the frame's first-hit features and the
// state's alone — no colour — and from that length how many times the frame's samples the pixel is given.  The geometry, the acceptance and the
// two sums are temporal.hpp's temporal_taps, as every stage that reads a history takes them.
//
// Everything is double.  + - * /, sqrt, floor and comparisons only, every product through unfused_mul() (adaptive.hpp), the order of every sum
// fixed here, so the device code, a g++ host build and a numpy restatement produce the same bits (tests/test_probe_cpu.py, tests/test_gpu_probe.py):
//   taps 00, 10, 01, 11 as temporal_taps takes them: wt = (i ? ax : 1 - ax) * (j ? ay : 1 - ay);  sw = sw + wt;  sl = sl + wt * prev_length[tp]
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

// One pixel of the call: temporal.hpp's taps and the length on them, no colour.  `prev_*` are not read without a history.
RT_HD ProbePixel probe_pixel(uint32_t w, uint32_t h, uint32_t x, uint32_t y, const TemporalParams& q, const SamplingParams& a, const double* normal,
                             const double* depth, const double* alpha, const double* prev_length, const double* prev_normal, const double* prev_depth,
                             const double* prev_alpha) {
    const TemporalTaps t = temporal_taps(w, h, x, y, q, normal, depth, alpha, prev_length, prev_normal, prev_depth, prev_alpha);
    ProbePixel out;
    out.length = t.blend ? t.sl / t.sw : 0.0; // 0: no history, a miss, a reset
    out.xy[0] = t.xy[0];
    out.xy[1] = t.xy[1];
    out.multiplier = probe_multiplier(a, out.length, alpha[size_t(y) * w + x] != 0.0);
    return out;
}

} // namespace rt
