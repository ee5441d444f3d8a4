// adaptive.hpp — the per-pixel noise estimate and stopping rule of rttnw_render_adaptive (include/rttnw_hip.h), shared by the device
// kernels (adaptive_kernels.hpp adaptive_resolve_kernel) and the host test harness (tests/adaptive_host).
//
// A pixel's chunk sums are independent estimates of its mean: chunk c holds n_c samples with mean m_c.  Over the K chunks of all
// passes so far (N = sum n_c samples) the state is folded chunk by chunk with the weighted incremental update (West 1979):
//     mu += (m_c - mu) * n_c / N,    M2 += n_c (m_c - mu_old) (m_c - mu_new)      =>  M2 = sum_c n_c (m_c - mu)^2,
// and the standard error of the pixel's mean is sqrt(M2 / ((K - 1) N)): an unbiased variance estimate for i.i.d. samples, the textbook
// sample standard error with one-sample chunks.  Everything is double, whatever the kernel's arithmetic type, and no product is fused
// into the add that follows it: every product goes through unfused_mul().  The contracted units are built with -ffp-contract=fast,
// which overrides `#pragma clang fp contract`, so the pragma alone would not do.  The host harness, the contracted and the strict
// device builds therefore fold to the same bits (tests/test_gpu_adaptive.py holds the device to the harness), and a pixel's stopping
// decision is a function of its own samples alone.  (The IEEE division and square root expand to fused steps of their own; those are
// correctly rounded, so they agree with the host's.)
#pragma once
#include "rt_types.hpp"
#include <math.h>

namespace rt {

// a * b, rounded once, as an opaque value: the compiler cannot fuse it into a following add or subtract (a register-only empty asm on
// the device; host builds do not contract, -std=c++17)
RT_HD double unfused_mul(double a, double b) {
    double p = a * b;
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+v"(p));
#endif
    return p;
}

struct AdaptivePixel {
    double mu[3]; // weighted mean of the chunk means, per channel
    double m2[3]; // sum_c n_c (m_c - mu)^2
    uint32_t n;   // samples folded (N)
    uint32_t k;   // chunks folded (K)
};

// Doubles of a pixel's record in the state of rttnw_render_adaptive_resume (include/rttnw_hip.h): its running sum r, g, b, then n, mu[3], k, m2[3], 0
constexpr uint32_t STATE_RECORD_DOUBLES = 12;

// Fold one chunk: its mean m[3] over n_c >= 1 samples.
RT_HD void adaptive_fold(AdaptivePixel& a, const double m[3], uint32_t n_c) {
    const uint32_t n_new = a.n + n_c;
    const double w = double(n_c) / double(n_new);
    for (int ch = 0; ch < 3; ++ch) {
        const double delta = m[ch] - a.mu[ch];
        a.mu[ch] = a.mu[ch] + unfused_mul(delta, w);
        a.m2[ch] = a.m2[ch] + unfused_mul(unfused_mul(double(n_c), delta), m[ch] - a.mu[ch]);
    }
    a.n = n_new;
    a.k += 1u;
}

// Standard error of the pixel's mean in channel ch; +inf with fewer than two chunks.
RT_HD double adaptive_stderr(const AdaptivePixel& a, int ch) {
    if (a.k < 2u) return INFINITY;
    return sqrt(a.m2[ch] / unfused_mul(double(a.k - 1u), double(a.n)));
}

// The criterion of one pass's end: stderr <= abs_error + rel_error * value in every channel (value: the pixel's mean as the render
// reports it).  A pixel with fewer than two chunks is never converged.
RT_HD bool adaptive_converged(const AdaptivePixel& a, const double value[3], double rel_error, double abs_error) {
    if (a.k < 2u) return false;
    for (int ch = 0; ch < 3; ++ch)
        if (!(adaptive_stderr(a, ch) <= abs_error + unfused_mul(rel_error, value[ch]))) return false;
    return true;
}

// Does the pixel take part in the next pass?  Not once it has the cap's samples, or meets the criterion.
RT_HD bool adaptive_active(const AdaptivePixel& a, const double value[3], double rel_error, double abs_error, uint32_t cap) {
    return a.n < cap && !adaptive_converged(a, value, rel_error, abs_error);
}

} // namespace rt
