// Host harness of rttnw_amd/csrc/temporal.hpp: rttnw_temporal_accumulate with the function the device kernel (temporal.hip) calls, pixel by pixel,
// behind the same Camera::new the library's host half runs (scene_lower.cpp make_camera), and a C interface for tests/test_temporal_cpu.py and
// tests/test_gpu_temporal.py.  th_camera_record hands a descriptor's record to the numpy restatement, whose arithmetic starts from it.
#include "../../include/rttnw_hip.h"
#include "../../rttnw_amd/csrc/scene_lower.hpp"
#include "../../rttnw_amd/csrc/temporal.hpp"

#include <cstring>

namespace {

rt::CameraRec<double> record_of(const rttnw_camera_desc* cam) {
    rt::CameraRec<double> c;
    rt::make_camera(cam->lookfrom, cam->lookat, cam->view_up, cam->vertical_fov, cam->aspect_ratio, cam->aperture, cam->focus_distance, cam->open_time,
                    cam->close_time, c);
    return c;
}

} // namespace

// out: origin, lower_left_corner, horizontal, vertical — 12 doubles
extern "C" void th_camera_record(const rttnw_camera_desc* cam, double* out) {
    const rt::CameraRec<double> c = record_of(cam);
    for (int k = 0; k < 3; ++k) {
        out[k] = c.origin[k];
        out[3 + k] = c.lower_left_corner[k];
        out[6 + k] = c.horizontal[k];
        out[9 + k] = c.vertical[k];
    }
}

// The entry point's arguments after its refusals: prev_linear == nullptr is "no history"; every output is optional.
extern "C" int th_temporal_accumulate(uint32_t w, uint32_t h, const rttnw_camera_desc* cam, const rttnw_camera_desc* prev_cam, const double* linear,
                                      const double* variance, const double* normal, const double* depth, const double* alpha, const double* prev_linear,
                                      const double* prev_variance, const double* prev_length, const double* prev_normal, const double* prev_depth,
                                      const double* prev_alpha, uint32_t max_history, double depth_tolerance, double normal_min, double* out, uint8_t* out_rgba8,
                                      double* out_variance, double* out_length, double* out_prev_xy) {
    const bool has_history = prev_linear != nullptr;
    if (max_history > rt::TEMPORAL_HISTORY_LIMIT || !(depth_tolerance >= 0.0) || !(normal_min >= -1.0 && normal_min <= 1.0)) return -1;
    if (has_history && (!prev_cam || !prev_length || !prev_normal || !prev_depth || !prev_alpha || (variance == nullptr) != (prev_variance == nullptr))) return -1;
    const rt::CameraRec<double> rec = record_of(cam);
    rt::CameraRec<double> prev_rec = {};
    if (has_history) prev_rec = record_of(prev_cam);
    const bool same = has_history && std::memcmp(cam, prev_cam, sizeof(rttnw_camera_desc)) == 0;
    const rt::TemporalParams prm = rt::temporal_params(rec, has_history ? &prev_rec : nullptr, same, max_history, depth_tolerance, normal_min, variance != nullptr);
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) {
            const rt::TemporalPixel px = rt::temporal_pixel(w, h, x, y, prm, linear, variance, normal, depth, alpha, prev_linear, prev_variance, prev_length,
                                                            prev_normal, prev_depth, prev_alpha);
            const size_t p = size_t(y) * w + x;
            for (int ch = 0; ch < 3; ++ch) {
                if (out) out[p * 3 + ch] = px.c[ch];
                if (out_rgba8) out_rgba8[p * 4 + ch] = rt::denoise_quantise(px.c[ch]);
                if (out_variance && variance) out_variance[p * 3 + ch] = px.v[ch];
            }
            if (out_rgba8) out_rgba8[p * 4 + 3] = 255;
            if (out_length) out_length[p] = px.length;
            if (out_prev_xy) {
                out_prev_xy[p * 2] = px.xy[0];
                out_prev_xy[p * 2 + 1] = px.xy[1];
            }
        }
    return 0;
}
