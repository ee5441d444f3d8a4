// nlm.hpp — the arithmetic of rttnw_denoise_nlm (include/rttnw_hip.h has the contract, DESIGN.md §10b the why), shared by the device kernels
// (nlm.hip) and the host test harness (tests/nlm_host): non-local means over two half-buffers (Rousselle, Knaus and Zwicker 2012) — the weights
// that average half A are patch distances measured in half B and the other way round, so no weight depends on the noise it averages.  No feature
// buffer is read.
//
// Everything is double.  + - * / and comparisons only — no sqrt in the filter (the RGBA8 output takes denoise_quantise's), no transcendental
// function — and every product goes through unfused_mul() (adaptive.hpp).  The order of every sum is fixed here, so the device code, a g++ host
// build and a numpy restatement produce the same bits (tests/test_nlm_cpu.py, tests/test_gpu_nlm.py):
//   the image is extended by clamping: a value "at" a coordinate outside the image is the value at the nearest pixel inside, for patch taps,
//     candidates and the variance's 3x3 alike, each coordinate clamped on its own (x = clamp(p + n), q = clamp(p + n + o))
//   pair variance   V(x) = (sum over the 3x3 around x, row-major, from 0.0, of ((a - b)^2 * 0.5)) / 9          per channel
//   delta_c(x, o)   = ((g_x - g_q)^2 - (V_x + min(V_x, V_q))) / (1e-10 + k^2 * (V_x + V_q)),  k^2 = k * k rounded once
//   delta(x, o)     = (delta_r + delta_g) + delta_b            (the sum over the channels: their mean is taken with the patch's, below)
//   row sum  R(x, o) = sum over nx = -f .. f, left to right, from 0.0, of delta(x + (nx, 0), o)
//   D(p, o)         = (sum over ny = -f .. f, top to bottom, from 0.0, of R(p + (0, ny), o)) / (3 (2f + 1)^2)   (one division per weight, not per delta)
//   w(p, o)         = (t t)(t t),  t = 1 / (1 + 0.25 * m),  m = 0 where D < 0, D otherwise;  w(p, 0) = 1 whatever D(p, 0) is
//   a'(p)           = (sum_o w_B(p, o) a(p + o)) / (sum_o w_B(p, o)),  both sums from 0.0 over oy = -r .. r (outer), ox = -r .. r (inner)
//   out = (a' + b') * 0.5;  error = ((a' - b') (a' - b')) * 0.25
// A value or a variance that is not finite is not special-cased: it propagates through every sum it enters (D < 0 is false for a NaN).
#pragma once
#include "denoise.hpp"

namespace rt {

constexpr uint32_t NLM_MAX_SEARCH_RADIUS = 16, NLM_MAX_PATCH_RADIUS = 4;
// The library defaults (a 0 in rttnw_nlm_params): Rousselle et al.'s patch of 7x7, their k of 0.45 widened for 8-sample halves
constexpr uint32_t NLM_SEARCH_RADIUS = 7, NLM_PATCH_RADIUS = 3;
constexpr double NLM_K = 0.7;
constexpr double NLM_EPS = 1e-10; // keeps delta's denominator positive where both variances are 0

// The call's parameters with the defaults resolved.
struct NlmParams {
    uint32_t r, f;
    double k2;         // k * k
    double patch_taps; // 3 (2f + 1)^2: the channels and taps a patch distance is the mean of
};
inline NlmParams nlm_params(uint32_t search_radius, uint32_t patch_radius, double k) {
    NlmParams q;
    q.r = search_radius == 0 ? NLM_SEARCH_RADIUS : search_radius;
    q.f = patch_radius == 0 ? NLM_PATCH_RADIUS : patch_radius;
    const double kk = k == 0.0 ? NLM_K : k;
    q.k2 = unfused_mul(kk, kk);
    q.patch_taps = double(3u * (2u * q.f + 1u) * (2u * q.f + 1u));
    return q;
}

// The call's input: row-major, top row first, w*h*3 each.  var_a == var_b (one array) when the call computed the pair variance itself.
struct NlmView {
    uint32_t width, height;
    const double *a, *b, *var_a, *var_b;
};

// coordinate c + d of an axis of n pixels, clamped to it
RT_HD uint32_t nlm_clamp(int c, int d, uint32_t n) {
    const int v = c + d;
    return v < 0 ? 0u : v >= int(n) ? n - 1u : uint32_t(v);
}

// The pair variance of pixel (x, y) in channel ch: the 3x3 mean of (a - b)^2 / 2
RT_HD double nlm_pair_variance(uint32_t width, uint32_t height, const double* a, const double* b, uint32_t x, uint32_t y, int ch) {
    double sum = 0.0;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const size_t q = (size_t(nlm_clamp(int(y), dy, height)) * width + nlm_clamp(int(x), dx, width)) * 3 + size_t(ch);
            const double d = a[q] - b[q];
            sum = sum + unfused_mul(unfused_mul(d, d), 0.5);
        }
    return sum / 9.0;
}

// delta_c: one channel of the pixel distance between x and q = x + o in one guide
RT_HD double nlm_delta_channel(double gx, double gq, double vx, double vq, double k2) {
    const double d = gx - gq;
    return (unfused_mul(d, d) - (vx + (vx < vq ? vx : vq))) / (NLM_EPS + unfused_mul(k2, vx + vq));
}
RT_HD double nlm_delta(double dr, double dg, double db) { return (dr + dg) + db; }

// w from the sum of the patch's row sums
RT_HD double nlm_weight(double column_sum, double patch_taps) {
    const double dist = column_sum / patch_taps;
    const double t = 1.0 / (1.0 + unfused_mul(0.25, dist < 0.0 ? 0.0 : dist));
    const double t2 = unfused_mul(t, t);
    return unfused_mul(t2, t2);
}

RT_HD double nlm_mean(double fa, double fb) { return unfused_mul(fa + fb, 0.5); }
RT_HD double nlm_error(double fa, double fb) {
    const double d = fa - fb;
    return unfused_mul(unfused_mul(d, d), 0.25);
}

// The device's tile: T x T output pixels per block, the guide and its variance staged in LDS with a halo of r + f (six planes of (T + 2(r + f))^2
// doubles) beside the two work arrays.  T = 32 where that fits the 160 KiB of a gfx950 CU — the defaults do, with 148 KiB —, T = 16 otherwise: at
// the largest radii the halo is 20 pixels, and (16 + 40)^2 x 6 doubles with the work arrays are 155 KiB.
constexpr uint32_t NLM_TILE_LARGE = 32, NLM_TILE_SMALL = 16;
constexpr size_t NLM_LDS_BYTES = 160u * 1024u;
constexpr size_t nlm_lds_bytes(uint32_t tile, uint32_t r, uint32_t f) {
    return (size_t(6) * (tile + 2 * (r + f)) * (tile + 2 * (r + f)) + size_t(tile + 2 * f) * (tile + 2 * f) + size_t(tile + 2 * f) * tile) * sizeof(double);
}
static_assert(nlm_lds_bytes(NLM_TILE_SMALL, NLM_MAX_SEARCH_RADIUS, NLM_MAX_PATCH_RADIUS) <= NLM_LDS_BYTES, "the small tile must fit the LDS at the largest radii");
static_assert(nlm_lds_bytes(NLM_TILE_LARGE, NLM_SEARCH_RADIUS, NLM_PATCH_RADIUS) <= NLM_LDS_BYTES, "the large tile must fit the LDS at the default radii");

// The filter kernel a call's radii take (nlm.hip nlm_plan_device): the tile, its dynamic LDS and the instantiation
struct NlmPlan {
    void (*filter)(NlmView, NlmParams, double*, double*);
    uint32_t tile;
    size_t lds_bytes;
};

// rttnw_denoise_nlm's device half (nlm.hip): host arrays in, host arrays out, blocking, on the current device.  Arguments were checked by the caller.
int nlm_device(uint32_t width, uint32_t height, const double* half_a, const double* half_b, const double* var_a, const double* var_b, const NlmParams& prm,
               double* out_linear_rgb, uint8_t* out_rgba8, double* out_half_a, double* out_half_b, double* out_error_rgb, double* kernel_ms);

} // namespace rt
