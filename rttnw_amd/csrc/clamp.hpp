// clamp.hpp — the arithmetic of rttnw_temporal_clamp (include/rttnw_hip.h has the contract, DESIGN.md §10b the why), shared by the device kernel
// (clamp.hip) and the host test harness (tests/clamp_host): neighbourhood variance clipping (Karis 2014; Salvi 2016) of the reprojected history in
// front of the blend of variance.hpp's stage A.  Stage S takes the mean and the standard deviation of THIS frame's colour over the window of
// variance_spatial — the same taps, drop rules and order, the weights denoise.hpp's denoise_edge_stops —, stage A' takes temporal.hpp's taps and
// the history's two means on them as variance.hpp's stage A does, clips the first into mean +- gamma * sd and blends.  One gather carries M1, M2
// and — for the rttnw_svgf handle, with feedback — the colour history H: the taps are taken once, and H is clipped into the same interval as M1.
//
// Everything is double.  + - * /, sqrt, floor and comparisons only, every product through unfused_mul() (adaptive.hpp), the order of every sum
// fixed here, so the device code, a g++ host build and a numpy restatement produce the same bits (tests/test_clamp_cpu.py, tests/test_gpu_clamp.py):
//   S:  w = w_n w_z over the window, dy outer, dx inner;  Sw = sum w;  mu = (sum w c') / Sw;  q = (sum w (c' c')) / Sw;  Sw > 0 false: mu = c,
//       q = c c;  sd = sqrt(pos(q - mu mu));  alpha == 0: mu = c, sd = 0;  lo = mu - gamma sd;  hi = mu + gamma sd
//   A': h1 = (sum wt m1') / W;  h2 = (sum wt m2') / W;  h1c = h1 < lo ? lo : (h1 > hi ? hi : h1) — a comparison with a NaN is false: nothing moves;
//       h2c = a branch was taken ? (h2 - h1 h1) + h1c h1c : h2;  out = (1 - a) * h1c + a * c;  out_m2 = (1 - a) * h2c + a * (c c)
#pragma once
#include "variance.hpp"

namespace rt {

// The library default (a 0 in rttnw_clamp_params): the literature's one standard deviation
constexpr double CLAMP_GAMMA = 1.0;

// Stage S's parameters with the defaults resolved
struct ClampParams {
    double gamma, sigma_depth;
    uint32_t radius, normal_squarings; // normal_squarings: as DenoiseParams
};
inline ClampParams clamp_params(uint32_t radius, double gamma, double sigma_normal, double sigma_depth) {
    const VarianceParams v = variance_params(0, radius, sigma_normal, sigma_depth);
    ClampParams q;
    q.gamma = gamma == 0.0 ? CLAMP_GAMMA : gamma;
    q.sigma_depth = v.sigma_depth;
    q.radius = v.radius;
    q.normal_squarings = v.normal_squarings;
    return q;
}

// What stage S reads, as a window onto the image, in VarianceView's terms: element (0, 0) of the view is image pixel (x0, y0), rows are `stride`
// pixels apart; channel ch of a three-channel quantity of view pixel q is at [q * pixel_step + ch * channel_step].  The whole image in global
// memory: x0 = y0 = 0, stride = width, steps 3 and 1.  The device's tile in LDS (clamp.hip): planes, steps 1 and the plane's size.
struct ClampView {
    const double *alpha, *depth, *normal, *colour;
    int x0, y0, stride, pixel_step, channel_step;
};
RT_HD int clamp_at(const ClampView& v, int x, int y) { return (y - v.y0) * v.stride + (x - v.x0); }

// Stage S, one pixel (x, y) of a w x h image: the weighted mean and standard deviation of this frame's colour over variance_spatial's window
RT_HD void clamp_statistics(const ClampView& v, const ClampParams& prm, int w, int h, int x, int y, double* mu, double* sd) {
    const int c = clamp_at(v, x, y);
    double n0[3], c0[3];
    for (int ch = 0; ch < 3; ++ch) {
        n0[ch] = v.normal[c * v.pixel_step + ch * v.channel_step];
        c0[ch] = v.colour[c * v.pixel_step + ch * v.channel_step];
    }
    if (v.alpha[c] == 0.0) { // the background is exact
        for (int ch = 0; ch < 3; ++ch) {
            mu[ch] = c0[ch];
            sd[ch] = 0.0;
        }
        return;
    }
    const double z0 = v.depth[c], az0 = z0 < 0.0 ? -z0 : z0;
    const int radius = int(prm.radius);
    double sw = 0.0, s1[3] = {0.0, 0.0, 0.0}, s2[3] = {0.0, 0.0, 0.0};
    for (int dy = -radius; dy <= radius; ++dy)
        for (int dx = -radius; dx <= radius; ++dx) {
            const int xx = x + dx, yy = y + dy;
            if (xx < 0 || yy < 0 || xx >= w || yy >= h) continue;
            const int q = clamp_at(v, xx, yy);
            if (v.alpha[q] == 0.0) continue;
            const int q3 = q * v.pixel_step;
            const EdgeStops e = denoise_edge_stops(n0, z0, az0, v.normal + q3, v.channel_step, v.depth[q], prm.normal_squarings, prm.sigma_depth);
            const double wt = unfused_mul(e.wn, e.wz);
            sw = sw + wt;
            for (int ch = 0; ch < 3; ++ch) {
                const double cq = v.colour[q3 + ch * v.channel_step];
                s1[ch] = s1[ch] + unfused_mul(wt, cq);
                s2[ch] = s2[ch] + unfused_mul(wt, unfused_mul(cq, cq));
            }
        }
    const bool any = sw > 0.0;
    for (int ch = 0; ch < 3; ++ch) {
        const double a1 = any ? s1[ch] / sw : c0[ch], a2 = any ? s2[ch] / sw : unfused_mul(c0[ch], c0[ch]);
        mu[ch] = a1;
        sd[ch] = sqrt(variance_pos(a2 - unfused_mul(a1, a1)));
    }
}

// Stage A', first half: temporal.hpp's taps and the three sums over them, left open: the window's bounds come between them and the blend.  sh is
// summed only with `feedback` (prev_history is then read) and is 0.0 otherwise; all three are 0.0 where `blend` is false.
struct ClampGathered : TemporalTaps {
    double s1[3], s2[3], sh[3];
};
RT_HD ClampGathered clamp_gather_pixel(uint32_t w, uint32_t h, uint32_t x, uint32_t y, const TemporalParams& q, bool feedback, const double* normal,
                                       const double* depth, const double* alpha, const double* prev_moment1, const double* prev_moment2,
                                       const double* prev_history, const double* prev_length, const double* prev_normal, const double* prev_depth,
                                       const double* prev_alpha) {
    ClampGathered g;
    static_cast<TemporalTaps&>(g) = temporal_taps(w, h, x, y, q, normal, depth, alpha, prev_length, prev_normal, prev_depth, prev_alpha);
    temporal_tap_sum(g, prev_moment1, g.s1);
    temporal_tap_sum(g, prev_moment2, g.s2);
    for (int ch = 0; ch < 3; ++ch) g.sh[ch] = 0.0;
    if (feedback) temporal_tap_sum(g, prev_history, g.sh);
    return g;
}

// One history mean into [lo, hi]; `moved`: one of the two branches was taken.  Every comparison with a NaN is false: a NaN stays, NaN bounds move nothing.
RT_HD double clamp_clip(double v, double lo, double hi, bool& moved) {
    if (v < lo) {
        moved = true;
        return lo;
    }
    if (v > hi) {
        moved = true;
        return hi;
    }
    moved = false;
    return v;
}

struct ClampAccumulated {
    double m1[3], m2[3], a[3], length; // a: the filter's input — the blend over the clipped H with `feedback`, m1 without
    uint8_t clipped;                   // bits 0 - 2: the channels of M1 that were clipped; bits 4 - 6: those of H
};

// Stage A', second half: the bounds from stage S's mean and deviation, the clip, the blend.  `cur`: this pixel's colour; mu and sd are read only
// where g.blend.
RT_HD ClampAccumulated clamp_finish_pixel(const ClampGathered& g, const TemporalParams& q, const ClampParams& prm, bool feedback, const double* cur,
                                          const double* mu, const double* sd) {
    ClampAccumulated out;
    double sq[3];
    for (int ch = 0; ch < 3; ++ch) { // this frame alone: no history, a miss, a reset
        out.m1[ch] = out.a[ch] = cur[ch];
        out.m2[ch] = sq[ch] = unfused_mul(cur[ch], cur[ch]);
    }
    out.length = 1.0;
    out.clipped = 0;
    if (!g.blend) return out;
    const TemporalBlend b = temporal_blend(g, q);
    for (int ch = 0; ch < 3; ++ch) {
        const double half = unfused_mul(prm.gamma, sd[ch]);
        const double lo = mu[ch] - half, hi = mu[ch] + half;
        const double h1 = g.s1[ch] / g.sw, h2 = g.s2[ch] / g.sw;
        bool moved;
        const double h1c = clamp_clip(h1, lo, hi, moved);
        double h2c = h2;
        if (moved) { // the history keeps its spread about the moved mean
            h2c = (h2 - unfused_mul(h1, h1)) + unfused_mul(h1c, h1c);
            out.clipped = uint8_t(out.clipped | (1u << ch));
        }
        out.m1[ch] = unfused_mul(b.wb, h1c) + unfused_mul(b.wa, cur[ch]);
        out.m2[ch] = unfused_mul(b.wb, h2c) + unfused_mul(b.wa, sq[ch]);
        if (feedback) {
            const double hc = clamp_clip(g.sh[ch] / g.sw, lo, hi, moved);
            if (moved) out.clipped = uint8_t(out.clipped | (16u << ch));
            out.a[ch] = unfused_mul(b.wb, hc) + unfused_mul(b.wa, cur[ch]);
        } else {
            out.a[ch] = out.m1[ch];
        }
    }
    out.length = b.n;
    return out;
}

// The device's blocks (clamp.hip): temporal.hip's, 64 pixels of a row by 4 rows; stage S's tile in LDS is the block and a halo of the radius, eight
// planes of doubles (alpha, depth, normal, colour): 44 800 bytes at radius 3, 55 296 at radius 4 — under the 64 KiB a kernel has without asking
constexpr uint32_t CLAMP_BLOCK_X = TEMPORAL_BLOCK_X, CLAMP_BLOCK_Y = TEMPORAL_BLOCK_Y, CLAMP_PLANES = 8;
constexpr size_t clamp_lds_bytes(uint32_t radius) {
    return size_t(CLAMP_BLOCK_X + 2 * radius) * (CLAMP_BLOCK_Y + 2 * radius) * CLAMP_PLANES * sizeof(double);
}
static_assert(clamp_lds_bytes(VARIANCE_MAX_RADIUS) <= 65536, "the clamp kernel's tile must fit the LDS a kernel has without asking");

} // namespace rt
