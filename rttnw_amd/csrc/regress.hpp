// regress.hpp — the arithmetic of rttnw_denoise_regress (include/rttnw_hip.h has the contract, DESIGN.md §10b the why), shared by the device
// kernels (regress.hip) and the host test harness (tests/regress_host): weighted first-order regression of colour on the first-hit features
// (Moon, Carr and Yoon 2014; Bitterli et al. 2016) with the cross-filtered non-local-means weights of nlm.hpp.  Where non-local means fits a
// constant to the candidates of a pixel, this fits colour = c0 + beta . x with x the candidate's features minus the centre's, and keeps c0.
//
// Everything is double.  + - * /, sqrt and comparisons only; every product goes through unfused_mul() (adaptive.hpp); every sum starts from 0.0
// and adds in the order stated here, so the device code, a g++ host build and a numpy restatement produce the same bits
// (tests/test_regress_cpu.py, tests/test_gpu_regress.py):
//   demodulation   a pixel with alpha != 0 and a channel with albedo > 1e-3 (denoise.hpp's rule): a, b / albedo, given variances / (albedo * albedo);
//                  the pair variance is then formed from the demodulated halves; a', b' * the centre's albedo at the end
//   weights        w(p, o) is nlm.hpp's, from the functions there; offsets row-major (oy outer, ox inner), the centre weighs 1
//   mask           m = features, or 0 where the centre's alpha == 0; with m != 0 a candidate whose clamped pixel has alpha == 0 enters no sum
//   x(q)           the selected components in the order albedo r g b, normal x y z, depth: feature(q) - feature(p); depth: (z_q - z_p) / z_p, z = depth / alpha
//   sums           s += w;  t_c += w y_c;  wx_i = w x_i;  b_i += wx_i;  A_ij += wx_i x_j (j <= i);  C_ic += wx_i y_c;  afterwards A_ii += ridge * s
//   solve          Cholesky row by row (acc = A_ji; acc -= L_jk L_ik, k < i in order; i < j: L_ji = acc / L_ii; i == j: acc > 0 must hold, L_jj = sqrt(acc)),
//                  u and G_c by forward substitution, uu = sum u_j u_j, uG_c = sum u_j G_jc, den = s - uu, value = (t_c - uG_c) / den
//   fallback       a pivot test that is false (a NaN included) or den >= 0.5 false: the zero-order value t_c / s over the same candidates
#pragma once
#include "nlm.hpp"

namespace rt {

// The library default of rttnw_regress_params.ridge (a 0 there): chosen from the sweep recorded in DESIGN.md §10b
constexpr double REGRESS_RIDGE = 1e-1;
constexpr uint32_t REGRESS_ALBEDO = 1u, REGRESS_NORMAL = 2u, REGRESS_DEPTH = 4u, REGRESS_ALL = 7u;
constexpr double REGRESS_MIN_DEN = 0.5; // den >= 1 in exact arithmetic (the centre weighs 1 with x = 0; the rest is Cauchy-Schwarz)

// d: the number of regressors a feature mask selects
RT_HD constexpr int regress_dim(uint32_t mask) { return ((mask & REGRESS_ALBEDO) ? 3 : 0) + ((mask & REGRESS_NORMAL) ? 3 : 0) + ((mask & REGRESS_DEPTH) ? 1 : 0); }

// The call's parameters with the defaults resolved.
struct RegressParams {
    NlmParams nlm;
    double ridge;
    uint32_t features, demodulate;
};
inline RegressParams regress_params(uint32_t search_radius, uint32_t patch_radius, double k, double ridge, uint32_t features, uint32_t demodulate) {
    RegressParams q;
    q.nlm = nlm_params(search_radius, patch_radius, k);
    q.ridge = ridge == 0.0 ? REGRESS_RIDGE : ridge;
    q.features = features;
    q.demodulate = demodulate != 0 ? 1u : 0u;
    return q;
}

// A pixel's features as the filter reads them: one 64-byte record, so that a candidate is one cache line.  Components whose array the call
// does not have (its bit is not set) are 0.0 and never read.
struct RegressRecord {
    double albedo[3], normal[3], z, alpha; // z = depth / alpha
};
static_assert(sizeof(RegressRecord) == 64, "one record per 64-byte line");
RT_HD RegressRecord regress_record(uint32_t mask, const double* albedo, const double* normal, const double* depth, const double* alpha, size_t p) {
    RegressRecord r;
    for (int c = 0; c < 3; ++c) {
        r.albedo[c] = (mask & REGRESS_ALBEDO) ? albedo[p * 3 + c] : 0.0;
        r.normal[c] = (mask & REGRESS_NORMAL) ? normal[p * 3 + c] : 0.0;
    }
    r.alpha = alpha[p];
    r.z = (mask & REGRESS_DEPTH) ? depth[p] / r.alpha : 0.0;
    return r;
}

// x(q) for the mask M, against the centre's record
template <uint32_t M> RT_HD void regress_x(const RegressRecord& p, const RegressRecord& q, double* x) {
    int i = 0;
    if (M & REGRESS_ALBEDO)
        for (int c = 0; c < 3; ++c) x[i++] = q.albedo[c] - p.albedo[c];
    if (M & REGRESS_NORMAL)
        for (int c = 0; c < 3; ++c) x[i++] = q.normal[c] - p.normal[c];
    if (M & REGRESS_DEPTH) x[i++] = (q.z - p.z) / p.z;
}

// The running sums of one pixel and direction.  A is the lower triangle, row-major: A_ij at i (i + 1) / 2 + j.
template <int D> struct RegressSums {
    static constexpr int N = D > 0 ? D : 1, NA = D > 0 ? D * (D + 1) / 2 : 1;
    double s, t[3], b[N], A[NA], C[N][3];
    RT_HD void clear() {
        s = 0.0;
        for (int c = 0; c < 3; ++c) t[c] = 0.0;
        for (int i = 0; i < N; ++i) {
            b[i] = 0.0;
            for (int c = 0; c < 3; ++c) C[i][c] = 0.0;
        }
        for (int i = 0; i < NA; ++i) A[i] = 0.0;
    }
    // NLM's two sums: every kept candidate enters these
    RT_HD void add_zero_order(double w, const double* y) {
        s = s + w;
        for (int c = 0; c < 3; ++c) t[c] = t[c] + unfused_mul(w, y[c]);
    }
    // ... and the first-order ones, for a pixel whose mask is not 0
    RT_HD void add_first_order(double w, const double* x, const double* y) {
        for (int i = 0; i < D; ++i) {
            const double wx = unfused_mul(w, x[i]);
            b[i] = b[i] + wx;
            for (int j = 0; j <= i; ++j) A[i * (i + 1) / 2 + j] = A[i * (i + 1) / 2 + j] + unfused_mul(wx, x[j]);
            for (int c = 0; c < 3; ++c) C[i][c] = C[i][c] + unfused_mul(wx, y[c]);
        }
    }
};

// Steps "after the loop" and 5: the ridge, the solve and the fallback.  `first_order` false: the pixel's mask is 0 (d = 0: uu = uG = 0.0).
// out[3]: the fitted value, or the zero-order one.  Returns whether the first-order value was used.  The sums are destroyed (L overwrites A).
template <int D> RT_HD bool regress_solve(RegressSums<D>& S, double ridge, bool first_order, double* out) {
    double uu = 0.0, uG[3] = {0.0, 0.0, 0.0};
    bool ok = true;
    if (D > 0 && first_order) {
        const double rs = unfused_mul(ridge, S.s);
        for (int i = 0; i < D; ++i) S.A[i * (i + 1) / 2 + i] = S.A[i * (i + 1) / 2 + i] + rs;
        for (int j = 0; j < D; ++j)
            for (int i = 0; i <= j; ++i) {
                double acc = S.A[j * (j + 1) / 2 + i];
                for (int k = 0; k < i; ++k) acc = acc - unfused_mul(S.A[j * (j + 1) / 2 + k], S.A[i * (i + 1) / 2 + k]);
                if (i < j) S.A[j * (j + 1) / 2 + i] = acc / S.A[i * (i + 1) / 2 + i];
                else {
                    if (!(acc > 0.0)) ok = false;
                    S.A[j * (j + 1) / 2 + j] = sqrt(acc);
                }
            }
        // forward substitution: u from b, G_c from C_c, in place
        for (int j = 0; j < D; ++j) {
            const double ljj = S.A[j * (j + 1) / 2 + j];
            double sum = 0.0;
            for (int k = 0; k < j; ++k) sum = sum + unfused_mul(S.A[j * (j + 1) / 2 + k], S.b[k]);
            S.b[j] = (S.b[j] - sum) / ljj;
            for (int c = 0; c < 3; ++c) {
                double sc = 0.0;
                for (int k = 0; k < j; ++k) sc = sc + unfused_mul(S.A[j * (j + 1) / 2 + k], S.C[k][c]);
                S.C[j][c] = (S.C[j][c] - sc) / ljj;
            }
        }
        for (int j = 0; j < D; ++j) {
            uu = uu + unfused_mul(S.b[j], S.b[j]);
            for (int c = 0; c < 3; ++c) uG[c] = uG[c] + unfused_mul(S.b[j], S.C[j][c]);
        }
    }
    const double den = S.s - uu;
    if (!(den >= REGRESS_MIN_DEN)) ok = false;
    for (int c = 0; c < 3; ++c) out[c] = ok ? (S.t[c] - uG[c]) / den : S.t[c] / S.s;
    return ok;
}

// The device's tile (regress.hip): nlm.hpp's plan — guide and variance staged in LDS with a halo of r + f — with one difference: the 60 running
// doubles of d = 7 do not fit the 128 registers a 1024-thread block leaves a lane, so masks with d >= 6 always take the 16-pixel tile (256
// threads), the others the 32-pixel tile where its LDS fits.
constexpr int REGRESS_LARGE_TILE_MAX_D = 4;
constexpr bool regress_mask_fits_large_tile(uint32_t mask) { return regress_dim(mask) <= REGRESS_LARGE_TILE_MAX_D; }
constexpr bool regress_tile_large(uint32_t mask, uint32_t r, uint32_t f) {
    return regress_mask_fits_large_tile(mask) && nlm_lds_bytes(NLM_TILE_LARGE, r, f) <= NLM_LDS_BYTES;
}

// rttnw_denoise_regress's device half (regress.hip): host arrays in, host arrays out (each optional), blocking, on the current device.
// Arguments were checked by the caller.
int regress_device(uint32_t width, uint32_t height, const double* half_a, const double* half_b, const double* var_a, const double* var_b,
                   const double* albedo, const double* normal, const double* depth, const double* alpha, const RegressParams& prm,
                   double* out_linear_rgb, uint8_t* out_rgba8, double* out_half_a, double* out_half_b, double* out_error_rgb, double* out_fit,
                   double* kernel_ms);

// ... and its kernels alone, in the shape of nlm_plan_device / nlm_passes_device: regress_plan_device picks the filter kernel of the call's mask
// and radii and its tile, and admits its dynamic LDS — before the caller starts its clock —, regress_passes_device enqueues the kernels on
// `stream` over buffers that are already on the device: nothing allocated, nothing copied, no wait.  d_var_a / d_var_b: the guides' variances,
// or both nullptr: the pair variance is then formed into the workspace's `pair`.  The feature arrays are read as the mask and `demodulate` ask
// (the others may be nullptr).  `at`: the prefix of an error's message.  rttnw_svgf_push_halves' spatial stage (svgf.hip).
struct RegressPlan {
    void (*filter)(NlmView, RegressParams, const RegressRecord*, const double*, const double*, double*, double*, uint8_t*, uint8_t*);
    uint32_t tile;
    size_t lds_bytes;
};
struct RegressWork {             // device buffers, per pixel:
    double *wa, *wb, *wva, *wvb; // 3 each: the demodulated halves and given variances (read and written only with demodulate)
    double* pair;                // 3: the pair variance (only without given variances)
    RegressRecord* rec;          // 1 record (only with a mask)
    double *fa, *fb;             // 3 each: the two fitted halves
    uint8_t *fit_a, *fit_b;      // 1 byte each: "the first-order value was used"
    double* out;                 // 3: their mean
    uint8_t* rgba;               // 4 bytes: its RGBA8
    double *err, *fit;           // 3, 1: the error estimate and the fit count
};
int regress_plan_device(const char* at, const RegressParams& prm, RegressPlan& plan);
#ifdef __HIPCC__
int regress_passes_device(const char* at, uint32_t width, uint32_t height, const double* d_a, const double* d_b, const double* d_var_a, const double* d_var_b,
                          const double* d_albedo, const double* d_normal, const double* d_depth, const double* d_alpha, const RegressParams& prm,
                          const RegressPlan& plan, const RegressWork& work, hipStream_t stream);
#endif

} // namespace rt
