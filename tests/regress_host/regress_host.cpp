// Host harness of rttnw_amd/csrc/regress.hpp: rttnw_denoise_regress with the functions the device kernels (regress.hip) call, in the order the
// header states, behind a C interface for tests/test_regress_cpu.py and tests/test_gpu_regress.py.  Whole-image maps per offset in place of
// the device's tiles, as tests/nlm_host: delta over the image and its patch halo, the row sums, then each pixel's weight and its sums.
//   -DREGRESS_HOST_MAIN   a stand-alone program (make sanitize): small frames through every mask, both variance modes and both tiles' radii
#include "../../rttnw_amd/csrc/regress.hpp"
#include <vector>

namespace {

using rt::RegressRecord;

// `src` regressed with the weights of `guide` (variance `var`): out w*h*3 (not remodulated), fit w*h (1 where the first-order value was used)
template <uint32_t M>
void cross_regress(uint32_t w, uint32_t h, const double* guide, const double* var, const double* src, const RegressRecord* rec, const rt::RegressParams& prm,
                   double* out, uint8_t* fit) {
    constexpr int D = rt::regress_dim(M);
    const int r = int(prm.nlm.r), f = int(prm.nlm.f), pw = int(w) + 2 * f, ph = int(h) + 2 * f;
    const size_t n = size_t(w) * h;
    std::vector<double> delta(size_t(pw) * ph), rows(size_t(w) * ph);
    std::vector<rt::RegressSums<D>> sums(n);
    for (auto& s : sums) s.clear();
    for (int oy = -r; oy <= r; ++oy)
        for (int ox = -r; ox <= r; ++ox) {
            const bool centre = ox == 0 && oy == 0;
            for (int ey = 0; !centre && ey < ph; ++ey)
                for (int ex = 0; ex < pw; ++ex) {
                    const size_t x = (size_t(rt::nlm_clamp(ey - f, 0, h)) * w + rt::nlm_clamp(ex - f, 0, w)) * 3;
                    const size_t q = (size_t(rt::nlm_clamp(ey - f, oy, h)) * w + rt::nlm_clamp(ex - f, ox, w)) * 3;
                    double d[3];
                    for (int ch = 0; ch < 3; ++ch) d[ch] = rt::nlm_delta_channel(guide[x + ch], guide[q + ch], var[x + ch], var[q + ch], prm.nlm.k2);
                    delta[size_t(ey) * pw + ex] = rt::nlm_delta(d[0], d[1], d[2]);
                }
            for (int ey = 0; !centre && ey < ph; ++ey)
                for (uint32_t x = 0; x < w; ++x) {
                    double sum = 0.0;
                    for (int k = 0; k <= 2 * f; ++k) sum = sum + delta[size_t(ey) * pw + x + k];
                    rows[size_t(ey) * w + x] = sum;
                }
            for (uint32_t y = 0; y < h; ++y)
                for (uint32_t x = 0; x < w; ++x) {
                    double wgt = 1.0;
                    if (!centre) {
                        double column = 0.0;
                        for (int k = 0; k <= 2 * f; ++k) column = column + rows[size_t(y + k) * w + x];
                        wgt = rt::nlm_weight(column, prm.nlm.patch_taps);
                    }
                    const size_t p = size_t(y) * w + x;
                    const size_t q = size_t(rt::nlm_clamp(int(y), oy, h)) * w + rt::nlm_clamp(int(x), ox, w);
                    const bool first_order = M != 0 && rec[p].alpha != 0.0;
                    if (first_order && rec[q].alpha == 0.0) continue; // a dropped candidate enters no sum
                    sums[p].add_zero_order(wgt, src + q * 3);
                    if (first_order) {
                        double xq[D > 0 ? D : 1];
                        rt::regress_x<M>(rec[p], rec[q], xq);
                        sums[p].add_first_order(wgt, xq, src + q * 3);
                    }
                }
        }
    for (size_t p = 0; p < n; ++p) fit[p] = rt::regress_solve<D>(sums[p], prm.ridge, M != 0 && rec[p].alpha != 0.0, out + p * 3) ? 1 : 0;
}

using CrossFn = void (*)(uint32_t, uint32_t, const double*, const double*, const double*, const RegressRecord*, const rt::RegressParams&, double*, uint8_t*);
const CrossFn CROSS[8] = {cross_regress<0>, cross_regress<1>, cross_regress<2>, cross_regress<3>, cross_regress<4>, cross_regress<5>, cross_regress<6>, cross_regress<7>};

} // namespace

extern "C" int rh_denoise_regress(uint32_t w, uint32_t h, const double* a, const double* b, const double* var_a, const double* var_b, const double* albedo,
                                  const double* normal, const double* depth, const double* alpha, uint32_t search_radius, uint32_t patch_radius, double k,
                                  double ridge, uint32_t features, uint32_t demodulate, double* out, uint8_t* out_rgba8, double* out_a, double* out_b,
                                  double* out_error, double* out_fit) {
    if (search_radius > rt::NLM_MAX_SEARCH_RADIUS || patch_radius > rt::NLM_MAX_PATCH_RADIUS || !(k >= 0.0) || !(ridge >= 0.0) || features > 7 ||
        (var_a == nullptr) != (var_b == nullptr)) return -1;
    if (features != 0 && (!alpha || ((features & 1) && !albedo) || ((features & 2) && !normal) || ((features & 4) && !depth))) return -1;
    if (demodulate != 0 && (!albedo || !alpha)) return -1;
    const rt::RegressParams prm = rt::regress_params(search_radius, patch_radius, k, ridge, features, demodulate);
    const size_t n = size_t(w) * h;
    std::vector<double> wa, wb, wva, wvb, pair, fa(n * 3), fb(n * 3);
    if (prm.demodulate) { // step 1
        wa.resize(n * 3), wb.resize(n * 3);
        if (var_a) wva.resize(n * 3), wvb.resize(n * 3);
        for (size_t i = 0; i < n * 3; ++i) {
            wa[i] = rt::denoise_demodulate(a[i], albedo[i], alpha[i / 3]);
            wb[i] = rt::denoise_demodulate(b[i], albedo[i], alpha[i / 3]);
            if (var_a) {
                wva[i] = rt::denoise_demodulate_variance(var_a[i], albedo[i], alpha[i / 3]);
                wvb[i] = rt::denoise_demodulate_variance(var_b[i], albedo[i], alpha[i / 3]);
            }
        }
        a = wa.data(), b = wb.data();
        if (var_a) var_a = wva.data(), var_b = wvb.data();
    }
    if (!var_a) {
        pair.resize(n * 3);
        for (size_t i = 0; i < n * 3; ++i) pair[i] = rt::nlm_pair_variance(w, h, a, b, uint32_t(i / 3 % w), uint32_t(i / 3 / w), int(i % 3));
        var_a = var_b = pair.data();
    }
    std::vector<RegressRecord> rec;
    if (features != 0) {
        rec.resize(n);
        for (size_t p = 0; p < n; ++p) rec[p] = rt::regress_record(features, albedo, normal, depth, alpha, p);
    }
    std::vector<uint8_t> fit_a(n), fit_b(n);
    CROSS[features](w, h, b, var_b, a, rec.data(), prm, fa.data(), fit_a.data());
    CROSS[features](w, h, a, var_a, b, rec.data(), prm, fb.data(), fit_b.data());
    for (size_t i = 0; i < n * 3; ++i) {
        if (prm.demodulate) {
            fa[i] = rt::denoise_remodulate(fa[i], albedo[i], alpha[i / 3]);
            fb[i] = rt::denoise_remodulate(fb[i], albedo[i], alpha[i / 3]);
        }
        const double c = rt::nlm_mean(fa[i], fb[i]);
        if (out) out[i] = c;
        if (out_rgba8) out_rgba8[i / 3 * 4 + i % 3] = rt::denoise_quantise(c);
        if (out_a) out_a[i] = fa[i];
        if (out_b) out_b[i] = fb[i];
        if (out_error) out_error[i] = rt::nlm_error(fa[i], fb[i]);
    }
    for (size_t i = 0; i < n; ++i) {
        if (out_rgba8) out_rgba8[i * 4 + 3] = 255;
        if (out_fit) out_fit[i] = double(fit_a[i] + fit_b[i]);
    }
    return 0;
}

#ifdef REGRESS_HOST_MAIN
#include <cstdio>
// A frame with an edge, a texture, a sky column (alpha 0), a pixel whose depth is 0 and fractional alphas; deterministic, no library RNG.
int main() {
    uint64_t state = 0x9E3779B97F4A7C15ull;
    const auto rnd = [&state]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return double(state >> 11) / 9007199254740992.0; };
    int runs = 0;
    const uint32_t sizes[3][2] = {{1, 1}, {3, 5}, {19, 17}}, radii[3][2] = {{1, 1}, {3, 2}, {16, 4}};
    for (const auto& size : sizes)
        for (const auto& rf : radii)
            for (uint32_t mask = 0; mask <= 7; ++mask)
                for (uint32_t flavour = 0; flavour < 4; ++flavour) {
                    const uint32_t w = size[0], h = size[1];
                    const size_t n = size_t(w) * h;
                    std::vector<double> a(n * 3), b(n * 3), va(n * 3), vb(n * 3), albedo(n * 3), normal(n * 3), depth(n), alpha(n);
                    for (size_t p = 0; p < n; ++p) {
                        alpha[p] = p % w == 2 ? 0.0 : p % 7 == 3 ? 0.5 : 1.0;
                        depth[p] = p == 5 ? 0.0 : (1.0 + 9.0 * rnd()) * alpha[p];
                        for (int c = 0; c < 3; ++c) {
                            albedo[p * 3 + c] = p % 11 == 0 ? 0.0 : 0.2 + 0.8 * rnd();
                            normal[p * 3 + c] = 2.0 * rnd() - 1.0;
                            const double e = (p % w < w / 2 ? 0.3 : 0.9) * albedo[p * 3 + c];
                            a[p * 3 + c] = e + 0.1 * rnd(), b[p * 3 + c] = e + 0.1 * rnd();
                            va[p * 3 + c] = 0.003 * rnd(), vb[p * 3 + c] = p % 5 == 0 ? 0.0 : 0.003 * rnd();
                        }
                    }
                    const bool given = flavour & 1, demodulate = flavour & 2;
                    std::vector<double> out(n * 3), oa(n * 3), ob(n * 3), err(n * 3), fit(n);
                    std::vector<uint8_t> rgba(n * 4);
                    const int rc = rh_denoise_regress(w, h, a.data(), b.data(), given ? va.data() : nullptr, given ? vb.data() : nullptr, albedo.data(),
                                                      normal.data(), depth.data(), alpha.data(), rf[0], rf[1], 0.0, flavour == 3 ? 1e-12 : 0.0, mask,
                                                      demodulate, out.data(), rgba.data(), oa.data(), ob.data(), err.data(), fit.data());
                    if (rc != 0) { std::printf("regress_host: call refused (%ux%u mask %u)\n", w, h, mask); return 1; }
                    for (size_t p = 0; p < n; ++p)
                        if (!(fit[p] == 0.0 || fit[p] == 1.0 || fit[p] == 2.0)) { std::printf("regress_host: fit out of range\n"); return 1; }
                    ++runs;
                }
    // the NULL feature arrays of property 1
    std::vector<double> a(15, 0.5), b(15, 0.25), out(15);
    if (rh_denoise_regress(5, 1, a.data(), b.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0.0, 0.0, 0, 0, out.data(), nullptr, nullptr, nullptr,
                           nullptr, nullptr) != 0) return 1;
    std::printf("regress_host: %d runs clean\n", runs + 1);
    return 0;
}
#endif
