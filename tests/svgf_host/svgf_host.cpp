// Host harness of rttnw_amd/csrc/svgf.hpp: one call of rttnw_svgf_push with the functions the device kernels call, pixel by pixel — ingest, the
// accumulation with its three quantities, variance.hpp's estimate, denoise.hpp's passes with the feedback tapped out of the pass loop, emit —
// behind the same Camera::new the library's host half runs, and a C interface for tests/test_svgf_cpu.py and tests/test_gpu_svgf.py.  The state is
// the caller's: the previous call's moment1_rgb, moment2_rgb, history_rgb, length and feature maps come in as arguments (prev_m1 == nullptr is the
// empty state), so the harness can be started from a made-up history.  With -DSVGF_HOST_MAIN it is a stand-alone program that runs four-frame
// chains over small and odd images under every setting, for a sanitizer (make sanitize).
#include "../../include/rttnw_hip.h"
#include "../../rttnw_amd/csrc/scene_lower.hpp"
#include "../../rttnw_amd/csrc/svgf.hpp"

#include <cstring>
#include <vector>

namespace {

rt::CameraRec<double> record_of(const rttnw_camera_desc* cam) {
    rt::CameraRec<double> c;
    rt::make_camera(cam->lookfrom, cam->lookat, cam->view_up, cam->vertical_fov, cam->aspect_ratio, cam->aperture, cam->focus_distance, cam->open_time,
                    cam->close_time, c);
    return c;
}

void copy_out(double* dst, const std::vector<double>& src) {
    if (dst) std::memcpy(dst, src.data(), src.size() * sizeof(double));
}

} // namespace

// The entry point's arguments after its refusals.  prev_h is read only with q->feedback_iterations > 0 and a state.
extern "C" int sh_svgf_push(uint32_t w, uint32_t h, const rttnw_svgf_params* q, const rttnw_camera_desc* cam, const rttnw_camera_desc* prev_cam,
                            const double* linear, const double* albedo, const double* normal, const double* depth, const double* alpha,
                            const double* prev_m1, const double* prev_m2, const double* prev_h, const double* prev_length, const double* prev_normal,
                            const double* prev_depth, const double* prev_alpha, const rttnw_svgf_out* out) {
    const bool has_state = prev_m1 != nullptr;
    if (q->d.iterations > rt::DENOISE_MAX_ITERATIONS || q->feedback_iterations > q->d.iterations || q->demodulate > 1 || q->v.radius > rt::VARIANCE_MAX_RADIUS) return -1;
    if (has_state && (!prev_cam || !prev_m2 || !prev_length || !prev_normal || !prev_depth || !prev_alpha)) return -1;
    const bool feedback = q->feedback_iterations > 0 && has_state;
    if (feedback && !prev_h) return -1;
    const rt::CameraRec<double> rec = record_of(cam);
    rt::CameraRec<double> prev_rec = {};
    if (has_state) prev_rec = record_of(prev_cam);
    const bool same = has_state && std::memcmp(cam, prev_cam, sizeof(rttnw_camera_desc)) == 0;
    const rt::TemporalParams prm = rt::temporal_params(rec, has_state ? &prev_rec : nullptr, same, q->t.max_history, q->t.depth_tolerance, q->t.normal_min, false);
    const rt::VarianceParams vprm = rt::variance_params(q->v.min_temporal, q->v.radius, q->v.sigma_normal, q->v.sigma_depth);
    const rt::DenoiseParams dprm = rt::denoise_params(q->d.sigma_luminance, q->d.sigma_normal, q->d.sigma_depth, true);
    const size_t npx = size_t(w) * h, n3 = npx * 3;

    // 0: ingest
    std::vector<double> c(n3), filter_albedo(n3);
    std::vector<uint8_t> flags(n3);
    for (size_t i = 0; i < n3; ++i) {
        c[i] = rt::svgf_ingest_value(q->demodulate != 0, linear[i], albedo[i], alpha[i / 3], flags[i]);
        filter_albedo[i] = q->demodulate ? 1.0 : albedo[i];
    }
    // 1, 2: accumulate, then estimate
    std::vector<double> m1(n3), m2(n3), acc(n3), length(npx), xy(npx * 2), var(n3);
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) {
            const rt::SvgfAccumulated px = rt::svgf_accumulate_pixel(w, h, x, y, prm, feedback, c.data(), normal, depth, alpha, prev_m1, prev_m2, prev_h,
                                                                     prev_length, prev_normal, prev_depth, prev_alpha);
            const size_t p = size_t(y) * w + x;
            for (int ch = 0; ch < 3; ++ch) {
                m1[p * 3 + ch] = px.m1[ch];
                m2[p * 3 + ch] = px.m2[ch];
                acc[p * 3 + ch] = px.a[ch];
            }
            length[p] = px.length;
            xy[p * 2] = px.xy[0];
            xy[p * 2 + 1] = px.xy[1];
        }
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x)
            rt::variance_estimate_pixel(w, h, x, y, vprm, m1.data(), m2.data(), length.data(), normal, depth, alpha, &var[(size_t(y) * w + x) * 3]);
    // 3, 4: the filter (denoise.hip's steps: prepare, the passes, finish), the feedback a finish step behind pass j
    const uint32_t iterations = q->d.iterations;
    std::vector<double> fc(acc), fv(var), fc2(n3), fv2(n3), hist, filtered(n3), filtered_var(n3);
    for (size_t i = 0; iterations > 0 && i < n3; ++i)
        rt::atrous_prepare_value<false>(true, &acc[i], &var[i], filter_albedo[i], alpha[i / 3], &fc[i], &fv[i]);
    for (uint32_t it = 0; it < iterations; ++it) {
        const rt::DenoiseView view{w, h, fc.data(), fv.data(), normal, depth, alpha};
        for (uint32_t y = 0; y < h; ++y)
            for (uint32_t x = 0; x < w; ++x) {
                const size_t o = (size_t(y) * w + x) * 3;
                rt::denoise_filter_pixel(view, dprm, x, y, 1u << it, &fc2[o], &fv2[o]);
            }
        fc.swap(fc2);
        fv.swap(fv2);
        if (it + 1 == q->feedback_iterations) {
            hist.resize(n3);
            for (size_t i = 0; i < n3; ++i) hist[i] = rt::denoise_remodulate(fc[i], filter_albedo[i], alpha[i / 3]);
        }
    }
    std::vector<uint8_t> scratch(4);
    for (size_t p = 0; p < npx; ++p)
        rt::atrous_finish_pixel<false>(true, iterations > 0, &fc[p * 3], &fv[p * 3], &filter_albedo[p * 3], alpha[p], &filtered[p * 3], scratch.data(),
                                       &filtered_var[p * 3]);
    if (!out) return 0;
    // 5: emit
    for (size_t i = 0; i < n3; ++i) {
        const double lin = rt::svgf_emit_value(filtered[i], albedo[i], flags[i]);
        if (out->linear_rgb) out->linear_rgb[i] = lin;
        if (out->accumulated_rgb) out->accumulated_rgb[i] = rt::svgf_emit_value(acc[i], albedo[i], flags[i]);
        if (out->rgba8) out->rgba8[i / 3 * 4 + i % 3] = rt::denoise_quantise(lin);
    }
    for (size_t p = 0; out->rgba8 && p < npx; ++p) out->rgba8[p * 4 + 3] = 255;
    copy_out(out->variance_rgb, var);
    copy_out(out->filtered_variance_rgb, filtered_var);
    copy_out(out->length, length);
    copy_out(out->prev_xy, xy);
    copy_out(out->moment1_rgb, m1);
    copy_out(out->moment2_rgb, m2);
    copy_out(out->history_rgb, q->feedback_iterations ? hist : m1);
    if (out->raw_rgb) std::memcpy(out->raw_rgb, linear, n3 * sizeof(double));
    if (out->albedo) std::memcpy(out->albedo, albedo, n3 * sizeof(double));
    if (out->normal) std::memcpy(out->normal, normal, n3 * sizeof(double));
    if (out->depth) std::memcpy(out->depth, depth, npx * sizeof(double));
    if (out->alpha) std::memcpy(out->alpha, alpha, npx * sizeof(double));
    if (out->image_ms) *out->image_ms = 0.0;
    return 0;
}

#ifdef SVGF_HOST_MAIN
#include <cstdio>

int main() {
    rttnw_camera_desc cams[4] = {};
    for (int k = 0; k < 4; ++k) {
        const double from[3] = {0.3 * (k < 3 ? k : 2), 0.2, 9.0}, at[3] = {0.0, 0.0, 0.0}, up[3] = {0.0, 1.0, 0.0};
        for (int i = 0; i < 3; ++i) {
            cams[k].lookfrom[i] = from[i];
            cams[k].lookat[i] = at[i];
            cams[k].view_up[i] = up[i];
        }
        cams[k].vertical_fov = 40.0;
        cams[k].focus_distance = 10.0;
        cams[k].close_time = 1.0;
    }
    const uint32_t sizes[4][2] = {{1, 1}, {3, 5}, {37, 29}, {70, 41}};
    uint64_t state = 88172645463325252ull;
    const auto uniform = [&state] { // xorshift64: values in [0, 1)
        state ^= state << 13;
        state ^= state >> 7;
        state ^= state << 17;
        return double(state >> 11) / 9007199254740992.0;
    };
    for (const auto& size : sizes)
        for (uint32_t feedback = 0; feedback <= 2; ++feedback)
            for (uint32_t demodulate = 0; demodulate <= 1; ++demodulate) {
                const uint32_t w = size[0], h = size[1];
                const size_t npx = size_t(w) * h;
                rttnw_svgf_params q = {};
                q.feedback_iterations = feedback;
                q.demodulate = demodulate;
                q.d.iterations = 3;
                q.v.min_temporal = 2;
                q.v.radius = 1 + (w + feedback) % 4;
                std::vector<double> lin(npx * 3), albedo(npx * 3), normal(npx * 3), depth(npx), alpha(npx), shown(npx * 3), var(npx * 3);
                std::vector<double> m1[2] = {lin, lin}, m2[2] = {lin, lin}, hist[2] = {lin, lin}, len[2] = {depth, depth};
                for (size_t p = 0; p < npx; ++p) {
                    alpha[p] = uniform() < 0.2 ? 0.0 : 1.0;
                    depth[p] = 9.0 * alpha[p];
                    normal[p * 3] = normal[p * 3 + 1] = 0.0;
                    normal[p * 3 + 2] = 1.0;
                    for (int ch = 0; ch < 3; ++ch) albedo[p * 3 + ch] = uniform() < 0.1 ? 5e-4 : 0.1 + uniform();
                }
                for (int k = 0; k < 4; ++k) {
                    for (double& v : lin) v = uniform();
                    const int cur = k & 1, old = cur ^ 1;
                    for (int j = 0; j < 4; ++j) cams[j].aspect_ratio = double(w) / double(h);
                    const bool st = k > 0;
                    rttnw_svgf_out out = {};
                    out.linear_rgb = shown.data();
                    out.variance_rgb = var.data();
                    out.moment1_rgb = m1[cur].data();
                    out.moment2_rgb = m2[cur].data();
                    out.history_rgb = hist[cur].data();
                    out.length = len[cur].data();
                    const int rc = sh_svgf_push(w, h, &q, &cams[k], st ? &cams[k - 1] : nullptr, lin.data(), albedo.data(), normal.data(), depth.data(),
                                                alpha.data(), st ? m1[old].data() : nullptr, st ? m2[old].data() : nullptr, st ? hist[old].data() : nullptr,
                                                st ? len[old].data() : nullptr, st ? normal.data() : nullptr, st ? depth.data() : nullptr,
                                                st ? alpha.data() : nullptr, &out);
                    if (rc != 0) return 1;
                    for (size_t p = 0; p < npx * 3; ++p)
                        if (!(var[p] >= 0.0) || !(shown[p] >= 0.0)) {
                            std::printf("%ux%u feedback %u demodulate %u frame %d: variance %g, colour %g\n", w, h, feedback, demodulate, k, var[p], shown[p]);
                            return 1;
                        }
                }
            }
    std::printf("svgf_host: ok\n");
    return 0;
}
#endif
