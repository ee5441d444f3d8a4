// feature_api.hpp — what feature_api.cpp (the extern "C" half of rttnw_render_features and rttnw_denoise) calls: the feature pass's launch
// code per arithmetic build (feature_kernels.hpp, instantiated in features_f32.hip / features_f64.hip / features_f64_strict.hip) and the
// denoiser's device half (denoise.hip).  Kept out of render_common.hpp: the render kernels' translation units do not read it.
#pragma once
#include "render_common.hpp"
#include "denoise.hpp"

namespace rt {

// rttnw_render_features' device half: host outputs (each optional), blocking.  Arguments were checked by the caller.
#define RT_FEATURE_ENTRY_POINTS(X, R)                                                                                                          \
    X(R, render_features_t, (::rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, double* out_albedo, double* out_normal, \
                             double* out_depth, double* out_alpha, rttnw_stats* stats))
RT_DECLARE_BUILDS(RT_FEATURE_ENTRY_POINTS)

// rttnw_denoise's device half (denoise.hip): host arrays in, host arrays out, blocking, on the current device.
int denoise_device(uint32_t width, uint32_t height, const double* linear_rgb, const double* variance_rgb, const double* albedo, const double* normal,
                   const double* depth, const double* alpha, uint32_t iterations, const DenoiseParams& prm, double* out_linear_rgb, uint8_t* out_rgba8,
                   double* out_variance_rgb, double* kernel_ms);

} // namespace rt
