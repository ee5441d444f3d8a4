// Host harness of rttnw_amd/csrc/probe.hpp: rttnw_temporal_probe with the function the device kernel (probe.hip) calls, pixel by pixel, behind the
// same Camera::new the library's host half runs (scene_lower.cpp make_camera), and a C interface for tests/test_probe_cpu.py and
// tests/test_gpu_probe.py.  With -DPROBE_HOST_MAIN it is a stand-alone program that runs three-frame chains over images smaller and larger than a
// device block and checks the multiplier's staircase, for a sanitizer (make sanitize).
#include "../../include/rttnw_hip.h"
#include "../../rttnw_amd/csrc/scene_lower.hpp"
#include "../../rttnw_amd/csrc/probe.hpp"

#include <cstring>
#include <vector>

namespace {

rt::CameraRec<double> record_of(const rttnw_camera_desc* cam) {
    rt::CameraRec<double> c;
    rt::make_camera(cam->lookfrom, cam->lookat, cam->view_up, cam->vertical_fov, cam->aspect_ratio, cam->aperture, cam->focus_distance, cam->open_time,
                    cam->close_time, c);
    return c;
}

} // namespace

// The entry point's arguments after its refusals: prev_length == nullptr is "no history"; every output is optional.
extern "C" int ph_temporal_probe(uint32_t w, uint32_t h, const rttnw_camera_desc* cam, const rttnw_camera_desc* prev_cam, const double* normal,
                                 const double* depth, const double* alpha, const double* prev_length, const double* prev_normal, const double* prev_depth,
                                 const double* prev_alpha, uint32_t max_history, double depth_tolerance, double normal_min, uint32_t boost, double fill,
                                 double* out_length, double* out_prev_xy, uint8_t* out_multiplier) {
    const bool has_history = prev_length != nullptr;
    if (max_history > rt::TEMPORAL_HISTORY_LIMIT || !(depth_tolerance >= 0.0) || !(normal_min >= -1.0 && normal_min <= 1.0)) return -1;
    if ((boost != 0 && boost != 1 && boost != 2 && boost != 4 && boost != 8) || !rt::temporal_finite(fill) || !(fill == 0.0 || fill >= 1.0)) return -1;
    if (has_history && (!prev_cam || !prev_normal || !prev_depth || !prev_alpha)) return -1;
    const rt::CameraRec<double> rec = record_of(cam);
    rt::CameraRec<double> prev_rec = {};
    if (has_history) prev_rec = record_of(prev_cam);
    const bool same = has_history && std::memcmp(cam, prev_cam, sizeof(rttnw_camera_desc)) == 0;
    const rt::TemporalParams prm = rt::temporal_params(rec, has_history ? &prev_rec : nullptr, same, max_history, depth_tolerance, normal_min, false);
    const rt::SamplingParams smp = rt::sampling_params(boost, fill);
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) {
            const rt::ProbePixel px = rt::probe_pixel(w, h, x, y, prm, smp, normal, depth, alpha, prev_length, prev_normal, prev_depth, prev_alpha);
            const size_t p = size_t(y) * w + x;
            if (out_length) out_length[p] = px.length;
            if (out_prev_xy) {
                out_prev_xy[p * 2] = px.xy[0];
                out_prev_xy[p * 2 + 1] = px.xy[1];
            }
            if (out_multiplier) out_multiplier[p] = uint8_t(px.multiplier);
        }
    return 0;
}

#ifdef PROBE_HOST_MAIN
#include <cstdio>

int main() {
    // the staircase of the contract at fill 8, boost 8
    const double lengths[7] = {0.0, 0.99, 1.0, 3.0, 3.0001, 7.0, 1e9};
    const uint32_t stairs[7] = {8, 4, 4, 2, 1, 1, 1};
    for (int k = 0; k < 7; ++k)
        if (rt::probe_multiplier(rt::sampling_params(0, 0.0), lengths[k], true) != stairs[k] || rt::probe_multiplier(rt::sampling_params(8, 8.0), lengths[k], false) != 1u) {
            std::printf("a length of %g gets %u\n", lengths[k], rt::probe_multiplier(rt::sampling_params(0, 0.0), lengths[k], true));
            return 1;
        }
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
    const uint32_t sizes[4][2] = {{1, 1}, {3, 5}, {37, 29}, {70, 41}}, boosts[4] = {1, 2, 4, 8};
    const double fills[4] = {1.0, 3.5, 8.0, 100.0};
    uint64_t state = 88172645463325252ull;
    const auto uniform = [&state] { // xorshift64: values in [0, 1)
        state ^= state << 13;
        state ^= state >> 7;
        state ^= state << 17;
        return double(state >> 11) / 9007199254740992.0;
    };
    size_t boosted = 0, plain = 0;
    for (const auto& size : sizes)
        for (const uint32_t boost : boosts)
            for (const double fill : fills) {
                const uint32_t w = size[0], h = size[1];
                const size_t npx = size_t(w) * h;
                std::vector<double> normal(npx * 3), depth(npx), alpha(npx), len[2] = {std::vector<double>(npx), std::vector<double>(npx)}, xy(npx * 2);
                std::vector<uint8_t> mult(npx);
                for (size_t p = 0; p < npx; ++p) {
                    alpha[p] = uniform() < 0.2 ? 0.0 : 1.0;
                    depth[p] = 9.0 * alpha[p];
                    normal[p * 3] = normal[p * 3 + 1] = 0.0;
                    normal[p * 3 + 2] = 1.0;
                }
                for (int k = 0; k < 3; ++k) {
                    const int cur = k & 1, old = cur ^ 1;
                    cams[k].aspect_ratio = double(w) / double(h);
                    if (k) cams[k - 1].aspect_ratio = cams[k].aspect_ratio;
                    const bool hist = k > 0;
                    const int rc = ph_temporal_probe(w, h, &cams[k], hist ? &cams[k - 1] : nullptr, normal.data(), depth.data(), alpha.data(),
                                                     hist ? len[old].data() : nullptr, hist ? normal.data() : nullptr, hist ? depth.data() : nullptr,
                                                     hist ? alpha.data() : nullptr, 0, 0.0, 0.0, boost, fill, len[cur].data(), xy.data(), mult.data());
                    if (rc != 0) return 1;
                    for (size_t p = 0; p < npx; ++p) {
                        const uint32_t m = mult[p];
                        if ((m != 1 && m != 2 && m != 4 && m != 8) || m > boost || (alpha[p] == 0.0 && m != 1) || !(len[cur][p] >= 0.0)) {
                            std::printf("%ux%u boost %u fill %g frame %d: a multiplier of %u beside a length of %g\n", w, h, boost, fill, k, m, len[cur][p]);
                            return 1;
                        }
                        boosted += m > 1;
                        plain += m == 1 && alpha[p] != 0.0;
                        len[cur][p] = len[cur][p] == 0.0 ? 1.0 : len[cur][p] + 1.0; // what the accumulation would keep: the next frame's history
                    }
                }
            }
    if (boosted == 0 || plain == 0) {
        std::printf("boosted hit pixels %zu, unboosted %zu\n", boosted, plain);
        return 1;
    }
    std::printf("probe_host: ok\n");
    return 0;
}
#endif
