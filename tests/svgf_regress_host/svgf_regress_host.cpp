// Host harness of the regression stage of the rttnw_svgf handle (rttnw_svgf_set_regress, include/rttnw_hip.h): one call of
// rttnw_svgf_push_halves with the functions the device kernels call, pixel by pixel — the halves' ingest, svgf.hpp's accumulation with its four
// quantities, variance.hpp's estimate, regress.hpp's filter over the accumulated halves (whole-image maps per offset in place of the device's
// tiles, as tests/regress_host), emit — behind the same Camera::new the library's host half runs, and a C interface for
// tests/test_svgf_regress_cpu.py and tests/test_gpu_svgf_regress.py.  The state is the caller's: the previous call's moment1_rgb, moment2_rgb,
// accumulated halves, length and feature maps come in as arguments (prev_m1 == nullptr is the empty state).  With -DSVGF_REGRESS_HOST_MAIN it is a
// stand-alone program that runs three-frame chains over small and odd images under every setting, for a sanitizer (make sanitize).
#include "../../include/rttnw_hip.h"
#include "../../rttnw_amd/csrc/scene_lower.hpp"
#include "../../rttnw_amd/csrc/svgf.hpp"

#include <cstring>
#include <vector>

namespace {

using rt::RegressRecord;

rt::CameraRec<double> record_of(const rttnw_camera_desc* cam) {
    rt::CameraRec<double> c;
    rt::make_camera(cam->lookfrom, cam->lookat, cam->view_up, cam->vertical_fov, cam->aspect_ratio, cam->aperture, cam->focus_distance, cam->open_time,
                    cam->close_time, c);
    return c;
}

void copy_out(double* dst, const std::vector<double>& src) {
    if (dst) std::memcpy(dst, src.data(), src.size() * sizeof(double));
}

// `src` regressed with the weights of `guide` (variance `var`): out w*h*3, fit w*h (1 where the first-order value was used)
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

// The entry point's arguments after its refusals, the handle's settings q and the stage's g and variance_source beside them.  out_* after `out`:
// what rttnw_svgf_halves copies out, each optional.
extern "C" int srh_svgf_push_halves(uint32_t w, uint32_t h, const rttnw_svgf_params* q, const rttnw_regress_params* g, uint32_t variance_source,
                                    const rttnw_camera_desc* cam, const rttnw_camera_desc* prev_cam, const double* half_a, const double* half_b,
                                    const double* albedo, const double* normal, const double* depth, const double* alpha, const double* prev_m1,
                                    const double* prev_m2, const double* prev_ha, const double* prev_hb, const double* prev_length,
                                    const double* prev_normal, const double* prev_depth, const double* prev_alpha, const rttnw_svgf_out* out,
                                    double* out_acc_a, double* out_acc_b, double* out_filtered_a, double* out_filtered_b, double* out_fit) {
    const bool has_state = prev_m1 != nullptr;
    if (q->feedback_iterations != 0 || q->demodulate > 1 || q->v.radius > rt::VARIANCE_MAX_RADIUS || variance_source > 1) return -1;
    if (g->search_radius > rt::NLM_MAX_SEARCH_RADIUS || g->patch_radius > rt::NLM_MAX_PATCH_RADIUS || !(g->k >= 0.0) || !(g->ridge >= 0.0) || g->features > 7 ||
        g->demodulate != 0) return -1;
    if (has_state && (!prev_cam || !prev_m2 || !prev_ha || !prev_hb || !prev_length || !prev_normal || !prev_depth || !prev_alpha)) return -1;
    const rt::CameraRec<double> rec = record_of(cam);
    rt::CameraRec<double> prev_rec = {};
    if (has_state) prev_rec = record_of(prev_cam);
    const bool same = has_state && std::memcmp(cam, prev_cam, sizeof(rttnw_camera_desc)) == 0;
    const rt::TemporalParams prm = rt::temporal_params(rec, has_state ? &prev_rec : nullptr, same, q->t.max_history, q->t.depth_tolerance, q->t.normal_min, false);
    const rt::VarianceParams vprm = rt::variance_params(q->v.min_temporal, q->v.radius, q->v.sigma_normal, q->v.sigma_depth);
    const rt::RegressParams gprm = rt::regress_params(g->search_radius, g->patch_radius, g->k, g->ridge, g->features, 0);
    const size_t npx = size_t(w) * h, n3 = npx * 3;

    // C and step 0
    std::vector<double> raw(n3), c(n3), ca(n3), cb(n3);
    std::vector<uint8_t> flags(n3);
    for (size_t i = 0; i < n3; ++i) {
        uint8_t same_flag;
        raw[i] = rt::svgf_halves_mean(half_a[i], half_b[i]);
        c[i] = rt::svgf_ingest_value(q->demodulate != 0, raw[i], albedo[i], alpha[i / 3], flags[i]);
        ca[i] = rt::svgf_ingest_value(q->demodulate != 0, half_a[i], albedo[i], alpha[i / 3], same_flag);
        cb[i] = rt::svgf_ingest_value(q->demodulate != 0, half_b[i], albedo[i], alpha[i / 3], same_flag);
    }
    // 1, 2: accumulate, then estimate
    std::vector<double> m1(n3), m2(n3), aa(n3), ab(n3), length(npx), xy(npx * 2), var(n3);
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) {
            const rt::SvgfAccumulatedHalves px = rt::svgf_accumulate_halves_pixel(w, h, x, y, prm, c.data(), ca.data(), cb.data(), normal, depth, alpha, prev_m1,
                                                                                  prev_m2, prev_ha, prev_hb, prev_length, prev_normal, prev_depth, prev_alpha);
            const size_t p = size_t(y) * w + x;
            for (int ch = 0; ch < 3; ++ch) {
                m1[p * 3 + ch] = px.m1[ch];
                m2[p * 3 + ch] = px.m2[ch];
                aa[p * 3 + ch] = px.a[ch];
                ab[p * 3 + ch] = px.b[ch];
            }
            length[p] = px.length;
            xy[p * 2] = px.xy[0];
            xy[p * 2 + 1] = px.xy[1];
        }
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x)
            rt::variance_estimate_pixel(w, h, x, y, vprm, m1.data(), m2.data(), length.data(), normal, depth, alpha, &var[(size_t(y) * w + x) * 3]);
    // 3: the filter (regress.hip's steps: the variance, the records, the two directions, finish)
    std::vector<double> half_var(n3), fa(n3), fb(n3), filtered(n3), error(n3), fit(npx);
    for (size_t i = 0; i < n3; ++i)
        half_var[i] = variance_source == 0 ? rt::svgf_half_variance(var[i])
                                           : rt::nlm_pair_variance(w, h, aa.data(), ab.data(), uint32_t(i / 3 % w), uint32_t(i / 3 / w), int(i % 3));
    std::vector<RegressRecord> records;
    if (gprm.features != 0) {
        records.resize(npx);
        for (size_t p = 0; p < npx; ++p) records[p] = rt::regress_record(gprm.features, albedo, normal, depth, alpha, p);
    }
    std::vector<uint8_t> fit_a(npx), fit_b(npx);
    CROSS[gprm.features](w, h, ab.data(), half_var.data(), aa.data(), records.data(), gprm, fa.data(), fit_a.data());
    CROSS[gprm.features](w, h, aa.data(), half_var.data(), ab.data(), records.data(), gprm, fb.data(), fit_b.data());
    for (size_t i = 0; i < n3; ++i) {
        filtered[i] = rt::nlm_mean(fa[i], fb[i]);
        error[i] = rt::nlm_error(fa[i], fb[i]);
    }
    for (size_t p = 0; p < npx; ++p) fit[p] = double(fit_a[p] + fit_b[p]);
    copy_out(out_acc_a, aa);
    copy_out(out_acc_b, ab);
    copy_out(out_filtered_a, fa);
    copy_out(out_filtered_b, fb);
    copy_out(out_fit, fit);
    if (!out) return 0;
    // 5: emit
    for (size_t i = 0; i < n3; ++i) {
        const double lin = rt::svgf_emit_value(filtered[i], albedo[i], flags[i]);
        if (out->linear_rgb) out->linear_rgb[i] = lin;
        if (out->accumulated_rgb) out->accumulated_rgb[i] = rt::svgf_emit_value(rt::svgf_halves_mean(aa[i], ab[i]), albedo[i], flags[i]);
        if (out->rgba8) out->rgba8[i / 3 * 4 + i % 3] = rt::denoise_quantise(lin);
    }
    for (size_t p = 0; out->rgba8 && p < npx; ++p) out->rgba8[p * 4 + 3] = 255;
    copy_out(out->variance_rgb, var);
    copy_out(out->filtered_variance_rgb, error);
    copy_out(out->length, length);
    copy_out(out->prev_xy, xy);
    copy_out(out->moment1_rgb, m1);
    copy_out(out->moment2_rgb, m2);
    copy_out(out->history_rgb, m1);
    copy_out(out->raw_rgb, raw);
    if (out->albedo) std::memcpy(out->albedo, albedo, n3 * sizeof(double));
    if (out->normal) std::memcpy(out->normal, normal, n3 * sizeof(double));
    if (out->depth) std::memcpy(out->depth, depth, npx * sizeof(double));
    if (out->alpha) std::memcpy(out->alpha, alpha, npx * sizeof(double));
    if (out->image_ms) *out->image_ms = 0.0;
    return 0;
}

#ifdef SVGF_REGRESS_HOST_MAIN
#include <cstdio>

int main() {
    rttnw_camera_desc cams[3] = {};
    for (int k = 0; k < 3; ++k) {
        const double from[3] = {0.02 * k, 0.0, 9.0}, at[3] = {0.02 * k, 0.0, 0.0}, up[3] = {0.0, 1.0, 0.0};
        for (int i = 0; i < 3; ++i) {
            cams[k].lookfrom[i] = from[i];
            cams[k].lookat[i] = at[i];
            cams[k].view_up[i] = up[i];
        }
        cams[k].vertical_fov = 40.0;
        cams[k].focus_distance = 9.0;
        cams[k].close_time = 1.0;
    }
    const uint32_t sizes[4][2] = {{1, 1}, {5, 3}, {45, 37}, {70, 9}};
    uint64_t state = 88172645463325252ull;
    const auto uniform = [&state] { // xorshift64: values in [0, 1)
        state ^= state << 13;
        state ^= state >> 7;
        state ^= state << 17;
        return double(state >> 11) / 9007199254740992.0;
    };
    int runs = 0;
    for (const auto& size : sizes)
        for (uint32_t features : {0u, 5u, 7u})
            for (uint32_t source = 0; source <= 1; ++source)
                for (uint32_t demodulate = 0; demodulate <= 1; ++demodulate) {
                    const uint32_t w = size[0], h = size[1];
                    const size_t npx = size_t(w) * h;
                    rttnw_svgf_params q = {};
                    q.demodulate = demodulate;
                    q.d.iterations = 3;
                    q.v.min_temporal = 2;
                    q.v.radius = 1 + (w + source) % 4;
                    rttnw_regress_params g = {};
                    g.search_radius = features == 5u ? 0 : 2; // (one mask at the default radii)
                    g.patch_radius = features == 5u ? 0 : 1;
                    g.features = features;
                    std::vector<double> a(npx * 3), b(npx * 3), albedo(npx * 3), normal(npx * 3), depth(npx), alpha(npx), shown(npx * 3), fit(npx);
                    std::vector<double> m1[2] = {a, a}, m2[2] = {a, a}, ha[2] = {a, a}, hb[2] = {a, a}, len[2] = {depth, depth};
                    for (size_t p = 0; p < npx; ++p) {
                        alpha[p] = uniform() < 0.2 ? 0.0 : 1.0;
                        depth[p] = 9.0 * alpha[p];
                        normal[p * 3] = normal[p * 3 + 1] = 0.0;
                        normal[p * 3 + 2] = 1.0;
                        for (int ch = 0; ch < 3; ++ch) albedo[p * 3 + ch] = uniform() < 0.1 ? 5e-4 : 0.1 + uniform();
                    }
                    for (int k = 0; k < 3; ++k) {
                        for (double& v : a) v = uniform();
                        for (double& v : b) v = uniform();
                        const int cur = k & 1, old = cur ^ 1;
                        for (int j = 0; j < 3; ++j) cams[j].aspect_ratio = double(w) / double(h);
                        const bool st = k > 0;
                        rttnw_svgf_out out = {};
                        out.linear_rgb = shown.data();
                        out.moment1_rgb = m1[cur].data();
                        out.moment2_rgb = m2[cur].data();
                        out.length = len[cur].data();
                        const int rc = srh_svgf_push_halves(w, h, &q, &g, source, &cams[k], st ? &cams[k - 1] : nullptr, a.data(), b.data(), albedo.data(),
                                                            normal.data(), depth.data(), alpha.data(), st ? m1[old].data() : nullptr,
                                                            st ? m2[old].data() : nullptr, st ? ha[old].data() : nullptr, st ? hb[old].data() : nullptr,
                                                            st ? len[old].data() : nullptr, st ? normal.data() : nullptr, st ? depth.data() : nullptr,
                                                            st ? alpha.data() : nullptr, &out, ha[cur].data(), hb[cur].data(), nullptr, nullptr, fit.data());
                        if (rc != 0) return 1;
                        for (size_t p = 0; p < npx; ++p)
                            if (!(fit[p] == 0.0 || fit[p] == 1.0 || fit[p] == 2.0) || !(shown[p * 3] == shown[p * 3])) {
                                std::printf("%ux%u features %u source %u demodulate %u frame %d: fit %g, colour %g\n", w, h, features, source, demodulate, k, fit[p],
                                            shown[p * 3]);
                                return 1;
                            }
                        ++runs;
                    }
                }
    std::printf("svgf_regress_host: %d calls clean\n", runs);
    return 0;
}
#endif
