// Host harness of rttnw_amd/csrc/clamp.hpp: rttnw_temporal_clamp with the functions the device kernel (clamp.hip) calls, pixel by pixel — stage S
// over the whole image in global memory, stage A' behind it, then variance.hpp's stage B over their outputs — behind the same Camera::new the
// library's host half runs (scene_lower.cpp make_camera), and a C interface for tests/test_clamp_cpu.py and tests/test_gpu_clamp.py.  With
// -DCLAMP_HOST_MAIN it is a stand-alone program that runs three-frame chains over images smaller and larger than a window, for a sanitizer
// (make sanitize).
#include "../../include/rttnw_hip.h"
#include "../../rttnw_amd/csrc/scene_lower.hpp"
#include "../../rttnw_amd/csrc/clamp.hpp"

#include <cstring>
#include <limits>
#include <vector>

namespace {

rt::CameraRec<double> record_of(const rttnw_camera_desc* cam) {
    rt::CameraRec<double> c;
    rt::make_camera(cam->lookfrom, cam->lookat, cam->view_up, cam->vertical_fov, cam->aspect_ratio, cam->aperture, cam->focus_distance, cam->open_time,
                    cam->close_time, c);
    return c;
}

} // namespace

// The entry point's arguments after its refusals: prev_linear == nullptr is "no history"; every output is optional.
extern "C" int ch_temporal_clamp(uint32_t w, uint32_t h, const rttnw_camera_desc* cam, const rttnw_camera_desc* prev_cam, const double* linear,
                                 const double* normal, const double* depth, const double* alpha, const double* prev_linear, const double* prev_moment2,
                                 const double* prev_length, const double* prev_normal, const double* prev_depth, const double* prev_alpha,
                                 uint32_t max_history, double depth_tolerance, double normal_min, uint32_t min_temporal, uint32_t radius, double sigma_normal,
                                 double sigma_depth, uint32_t clamp_radius, double gamma, double clamp_sigma_normal, double clamp_sigma_depth, double* out,
                                 uint8_t* out_rgba8, double* out_moment2, double* out_length, double* out_prev_xy, double* out_variance, double* out_mean,
                                 double* out_sd, uint8_t* out_clipped) {
    const bool has_history = prev_linear != nullptr;
    if (max_history > rt::TEMPORAL_HISTORY_LIMIT || !(depth_tolerance >= 0.0) || !(normal_min >= -1.0 && normal_min <= 1.0)) return -1;
    if (min_temporal == 1 || min_temporal > rt::TEMPORAL_HISTORY_LIMIT || radius > rt::VARIANCE_MAX_RADIUS || !(sigma_normal >= 0.0) || !(sigma_depth >= 0.0)) return -1;
    if (clamp_radius > rt::VARIANCE_MAX_RADIUS || !(gamma >= 0.0) || !(clamp_sigma_normal >= 0.0) || !(clamp_sigma_depth >= 0.0)) return -1;
    if (has_history && (!prev_cam || !prev_moment2 || !prev_length || !prev_normal || !prev_depth || !prev_alpha)) return -1;
    const rt::CameraRec<double> rec = record_of(cam);
    rt::CameraRec<double> prev_rec = {};
    if (has_history) prev_rec = record_of(prev_cam);
    const bool same = has_history && std::memcmp(cam, prev_cam, sizeof(rttnw_camera_desc)) == 0;
    const rt::TemporalParams prm = rt::temporal_params(rec, has_history ? &prev_rec : nullptr, same, max_history, depth_tolerance, normal_min, false);
    const rt::VarianceParams vprm = rt::variance_params(min_temporal, radius, sigma_normal, sigma_depth);
    const rt::ClampParams kprm = rt::clamp_params(clamp_radius, gamma, clamp_sigma_normal, clamp_sigma_depth);
    const rt::ClampView view = {alpha, depth, normal, linear, 0, 0, int(w), 3, 1};
    const size_t npx = size_t(w) * h;
    std::vector<double> m1(npx * 3), m2(npx * 3), length(npx);
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) {
            const size_t p = size_t(y) * w + x;
            double mu[3], sd[3];
            rt::clamp_statistics(view, kprm, int(w), int(h), int(x), int(y), mu, sd);
            const rt::ClampGathered g = rt::clamp_gather_pixel(w, h, x, y, prm, false, normal, depth, alpha, prev_linear, prev_moment2, nullptr, prev_length,
                                                               prev_normal, prev_depth, prev_alpha);
            const rt::ClampAccumulated px = rt::clamp_finish_pixel(g, prm, kprm, false, linear + p * 3, mu, sd);
            for (int ch = 0; ch < 3; ++ch) {
                m1[p * 3 + ch] = px.m1[ch];
                m2[p * 3 + ch] = px.m2[ch];
                if (out) out[p * 3 + ch] = px.m1[ch];
                if (out_rgba8) out_rgba8[p * 4 + ch] = rt::denoise_quantise(px.m1[ch]);
                if (out_moment2) out_moment2[p * 3 + ch] = px.m2[ch];
                if (out_mean) out_mean[p * 3 + ch] = mu[ch];
                if (out_sd) out_sd[p * 3 + ch] = sd[ch];
            }
            length[p] = px.length;
            if (out_rgba8) out_rgba8[p * 4 + 3] = 255;
            if (out_length) out_length[p] = px.length;
            if (out_prev_xy) {
                out_prev_xy[p * 2] = g.xy[0];
                out_prev_xy[p * 2 + 1] = g.xy[1];
            }
            if (out_clipped) out_clipped[p] = px.clipped;
        }
    if (out_variance)
        for (uint32_t y = 0; y < h; ++y)
            for (uint32_t x = 0; x < w; ++x)
                rt::variance_estimate_pixel(w, h, x, y, vprm, m1.data(), m2.data(), length.data(), normal, depth, alpha, out_variance + (size_t(y) * w + x) * 3);
    return 0;
}

#ifdef CLAMP_HOST_MAIN
#include <cstdio>

int main() {
    rttnw_camera_desc cams[3] = {};
    for (int k = 0; k < 3; ++k) {
        const double from[3] = {0.3 * (k < 2 ? k : 1), 0.2, 9.0}, at[3] = {0.0, 0.0, 0.0}, up[3] = {0.0, 1.0, 0.0};
        for (int i = 0; i < 3; ++i) {
            cams[k].lookfrom[i] = from[i];
            cams[k].lookat[i] = at[i];
            cams[k].view_up[i] = up[i];
        }
        cams[k].vertical_fov = 40.0;
        cams[k].aperture = 0.0;
        cams[k].focus_distance = 10.0;
        cams[k].close_time = 1.0;
    }
    const uint32_t sizes[4][2] = {{1, 1}, {3, 5}, {37, 29}, {70, 41}};
    const double gammas[3] = {0.25, 1.0, std::numeric_limits<double>::infinity()};
    uint64_t state = 88172645463325252ull;
    const auto uniform = [&state] { // xorshift64: values in [0, 1)
        state ^= state << 13;
        state ^= state >> 7;
        state ^= state << 17;
        return double(state >> 11) / 9007199254740992.0;
    };
    for (const auto& size : sizes)
        for (uint32_t radius = 1; radius <= rt::VARIANCE_MAX_RADIUS; ++radius)
            for (const double gamma : gammas) {
                const uint32_t w = size[0], h = size[1];
                const size_t npx = size_t(w) * h;
                std::vector<double> lin(npx * 3), normal(npx * 3), depth(npx), alpha(npx);
                std::vector<double> out[2] = {std::vector<double>(npx * 3), std::vector<double>(npx * 3)}, m2[2] = {out[0], out[0]};
                std::vector<double> len[2] = {std::vector<double>(npx), std::vector<double>(npx)}, xy(npx * 2), var(npx * 3), mean(npx * 3), sd(npx * 3);
                std::vector<uint8_t> rgba(npx * 4), clipped(npx);
                for (size_t p = 0; p < npx; ++p) {
                    alpha[p] = uniform() < 0.2 ? 0.0 : 1.0;
                    depth[p] = 9.0 * alpha[p];
                    normal[p * 3] = normal[p * 3 + 1] = 0.0;
                    normal[p * 3 + 2] = 1.0;
                }
                size_t moved = 0;
                for (int k = 0; k < 3; ++k) {
                    for (double& v : lin) v = uniform();
                    const int cur = k & 1, old = cur ^ 1;
                    cams[k].aspect_ratio = double(w) / double(h);
                    if (k) cams[k - 1].aspect_ratio = cams[k].aspect_ratio;
                    const bool hist = k > 0;
                    const int rc = ch_temporal_clamp(w, h, &cams[k], hist ? &cams[k - 1] : nullptr, lin.data(), normal.data(), depth.data(), alpha.data(),
                                                     hist ? out[old].data() : nullptr, hist ? m2[old].data() : nullptr, hist ? len[old].data() : nullptr,
                                                     hist ? normal.data() : nullptr, hist ? depth.data() : nullptr, hist ? alpha.data() : nullptr, 0, 0.0, 0.0, 2,
                                                     radius, 0.0, 0.0, radius, gamma, 0.0, 0.0, out[cur].data(), rgba.data(), m2[cur].data(), len[cur].data(),
                                                     xy.data(), var.data(), mean.data(), sd.data(), clipped.data());
                    if (rc != 0) return 1;
                    for (size_t p = 0; p < npx; ++p) moved += clipped[p] != 0;
                    for (size_t p = 0; p < npx * 3; ++p)
                        if (!(var[p] >= 0.0) || !(sd[p] >= 0.0)) {
                            std::printf("%ux%u radius %u gamma %g frame %d: a variance of %g, a deviation of %g\n", w, h, radius, gamma, k, var[p], sd[p]);
                            return 1;
                        }
                }
                if (gamma > 1e300 && moved != 0) {
                    std::printf("%ux%u radius %u: gamma +inf clipped %zu pixels\n", w, h, radius, moved);
                    return 1;
                }
            }
    std::printf("clamp_host: ok\n");
    return 0;
}
#endif
