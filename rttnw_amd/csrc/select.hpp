// select.hpp — the arithmetic of rttnw_denoise_select (include/rttnw_hip.h has the contract, DESIGN.md §10b the why), shared by the device kernels
// (select.hip) and the host test harness (tests/select_host): a per-pixel choice between the feature-guided à-trous filter (denoise.hpp) and
// non-local means over two half-buffers (nlm.hpp), after the selection step of Rousselle, Knaus and Zwicker 2012.  Each half is filtered by both
// filters; a filtered half is scored against the OTHER, raw half, which is an independent estimate of the same frame — the raw half's own noise
// enters both filters' scores alike and cancels in their difference.
//
// Everything is double.  + - * / and comparisons only, every product through unfused_mul() (adaptive.hpp), the order of every sum fixed here, so
// the device code, a g++ host build and a numpy restatement produce the same bits (tests/test_select_cpu.py, tests/test_gpu_select.py):
//   Fa, Fb = rttnw_denoise of each half;  Na, Nb = rttnw_denoise_nlm's two cross-filtered halves;  a, b = the raw halves
//   tF_c   = (Fa_c - b_c)^2 + (Fb_c - a_c)^2;   E_F = (tF_r + tF_g) + tF_b;   E_N likewise from Na, Nb
//   d      = (E_F - E_N) / (1e-10 + (E_F + E_N))                       in [-1, 1]: a bright region's errors do not outvote its neighbours
//   windows  coordinates clamped to the image, each on its own, as in nlm.hpp
//   R(x, y) = sum over ox = -s .. s, left to right, from 0.0, of d(clamp(x + ox), y);  S(p) = sum over oy = -s .. s, top to bottom, from 0.0, of
//            R(x, clamp(y + oy));  m(p) = 1.0 where S(p) > margin * double((2s+1)^2) (the product rounded once), otherwise — a NaN S too — 0.0
//   beta(p) = (the same two-stage clamped sum of m with radius t) / double((2t+1)^2)
//   blend(n, f) = f where beta == 0, n where beta == 1, otherwise beta * n + (1.0 - beta) * f (two products, one sum)
//   out = blend(N, F), F = (Fa + Fb) * 0.5, N = (Na + Nb) * 0.5;  error = ((A - B)(A - B)) * 0.25, A = blend(Na, Fa), B = blend(Nb, Fb)
#pragma once
#include "nlm.hpp"

namespace rt {

constexpr uint32_t SELECT_MAX_ERROR_RADIUS = 16, SELECT_MAX_BLEND_RADIUS = 8;
// The library defaults (a 0 radius, use_default_margin != 0 in rttnw_select_params); DESIGN.md §10b says why the margin is not 0
constexpr uint32_t SELECT_ERROR_RADIUS = 5, SELECT_BLEND_RADIUS = 2;
constexpr double SELECT_MARGIN = 0.01;
constexpr double SELECT_EPS = 1e-10; // keeps d's denominator positive where both errors are 0

// The call's parameters with the defaults resolved.
struct SelectParams {
    uint32_t s, t;
    double threshold;  // margin * double((2s+1)^2): what S(p) must exceed for non-local means to be chosen
    double blend_taps; // double((2t+1)^2)
};
inline SelectParams select_params(uint32_t error_radius, uint32_t blend_radius, double margin, bool use_default_margin) {
    SelectParams q;
    q.s = error_radius == 0 ? SELECT_ERROR_RADIUS : error_radius;
    q.t = blend_radius == 0 ? SELECT_BLEND_RADIUS : blend_radius;
    q.threshold = unfused_mul(use_default_margin ? SELECT_MARGIN : margin, double((2u * q.s + 1u) * (2u * q.s + 1u)));
    q.blend_taps = double((2u * q.t + 1u) * (2u * q.t + 1u));
    return q;
}

// E of one filter at one pixel: its filtered halves fa, fb against the raw halves of the other side, b and a (3 doubles each)
RT_HD double select_cross_error(const double* fa, const double* fb, const double* a, const double* b) {
    double t[3];
    for (int ch = 0; ch < 3; ++ch) {
        const double da = fa[ch] - b[ch], db = fb[ch] - a[ch];
        t[ch] = unfused_mul(da, da) + unfused_mul(db, db);
    }
    return (t[0] + t[1]) + t[2];
}
// d: the normalised error difference, positive where non-local means is the closer one
RT_HD double select_difference(double e_feature, double e_nlm) { return (e_feature - e_nlm) / (SELECT_EPS + (e_feature + e_nlm)); }
// m from the window sum S (false for a NaN: the feature filter)
RT_HD double select_choice(double window_sum, double threshold) { return window_sum > threshold ? 1.0 : 0.0; }
RT_HD double select_beta(double window_sum, double blend_taps) { return window_sum / blend_taps; }
// The branches keep a non-finite value of the filter that was not chosen out of the pixel
RT_HD double select_blend(double beta, double n, double f) {
    if (beta == 0.0) return f;
    if (beta == 1.0) return n;
    return unfused_mul(beta, n) + unfused_mul(1.0 - beta, f);
}

// The device's tile (select.hip): 32x32 output pixels per block; d staged with a halo of s + t, then its row sums, m on the tile and a halo of
// t, and m's row sums, all in LDS: at the largest radii (32 + 48)^2 + 80 * 48 + 48^2 + 48 * 32 doubles = 110 KiB, at the defaults 49 KiB.
constexpr uint32_t SELECT_TILE = 32;
constexpr size_t select_lds_bytes(uint32_t s, uint32_t t) {
    return (size_t(SELECT_TILE + 2 * (s + t)) * (SELECT_TILE + 2 * (s + t)) + size_t(SELECT_TILE + 2 * (s + t)) * (SELECT_TILE + 2 * t) +
            size_t(SELECT_TILE + 2 * t) * (SELECT_TILE + 2 * t) + size_t(SELECT_TILE + 2 * t) * SELECT_TILE) * sizeof(double);
}
static_assert(select_lds_bytes(SELECT_MAX_ERROR_RADIUS, SELECT_MAX_BLEND_RADIUS) <= NLM_LDS_BYTES, "the tile must fit the LDS at the largest radii");

} // namespace rt
