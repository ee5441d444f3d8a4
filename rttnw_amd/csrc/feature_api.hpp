// feature_api.hpp — what feature_api.cpp (the extern "C" half of rttnw_render_features and of the nine image-filter entry points), svgf.hip (the
// rttnw_svgf handle) and render_adaptive_api.cpp (the filtering adaptive renders) share: the feature pass's launch code per arithmetic build
// (feature_kernels.hpp, instantiated in features_f32.hip / features_f64.hip / features_f64_strict.hip); the device halves of rttnw_denoise and
// rttnw_reconstruct (denoise.hip), rttnw_denoise_nlm (nlm.hip), rttnw_denoise_select (select.hip), rttnw_temporal_accumulate (temporal.hip),
// rttnw_temporal_variance (variance.hip), rttnw_temporal_clamp (clamp.hip) and rttnw_temporal_probe (probe.hip), each as a blocking call on host
// arrays (on filter_call.hpp's scaffold) and as its kernels alone on device buffers; and what the entry points refuse for a parameter block
// (feature_api.cpp).  rttnw_denoise_regress's device half is declared in regress.hpp.
// Kept out of render_common.hpp: the render kernels' translation units do not read it.
#pragma once
#include "render_common.hpp"
#include "denoise.hpp"
#include "nlm.hpp"
#include "select.hpp"
#include "temporal.hpp"
#include "variance.hpp"
#include "clamp.hpp"
#include "probe.hpp"

namespace rt {

// ---- Refusals (feature_api.cpp).  One function per parameter block, for every entry point that takes the block, on its own or inside a struct of
// its own: 0, or RTTNW_ERR_INVALID behind the message "<call>: ..." that names the field.  `field`: how the caller's signature names the block,
// "t->", "q->t.", "dn->", "g->denoise."; a limit or a text lives here once.
int refuse(const char* call, const std::string& what); // RTTNW_ERR_INVALID behind "<call>: <what>"
int image_size_refused(const char* call, uint32_t width, uint32_t height); // an empty image, or more pixels than the filters' 32-bit indices take
int temporal_refuse_params(const char* call, const char* field, const rttnw_temporal_params& t);
int variance_refuse_params(const char* call, const char* field, const rttnw_variance_params& v);
int denoise_refuse_params(const char* call, const char* field, const rttnw_denoise_params& d);
int nlm_refuse_params(const char* call, const char* field, const rttnw_nlm_params& d);
int regress_refuse_params(const char* call, const rttnw_regress_params* g);   // a NULL g among them: rttnw_denoise_regress, rttnw_svgf_set_regress
int clamp_refuse_params(const char* call, const rttnw_clamp_params* k);       // a NULL k among them: rttnw_temporal_clamp, rttnw_svgf_set_clamp
int sampling_refuse_params(const char* call, const rttnw_sampling_params* a); // a NULL a among them: rttnw_temporal_probe, rttnw_svgf_set_sampling
// The reprojection of a frame seen through `cam` into a history seen through `prev_cam` (nullptr: no history), under a checked t
TemporalParams history_temporal_params(const rttnw_camera_desc* cam, const rttnw_camera_desc* prev_cam, const rttnw_temporal_params& t, bool has_variance);

// rttnw_render_features' device half: host outputs (each optional), blocking — and the same pass with its maps left on the device
// (feature_kernels.hpp).  Arguments were checked by the caller.
#define RT_FEATURE_ENTRY_POINTS(X, R)                                                                                                          \
    X(R, render_features_t, (::rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, double* out_albedo, double* out_normal, \
                             double* out_depth, double* out_alpha, rttnw_stats* stats))                                                       \
    X(R, render_features_device_t, (::rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, double* d_maps, hipStream_t stream))
RT_DECLARE_BUILDS(RT_FEATURE_ENTRY_POINTS)

// rttnw_denoise's and rttnw_reconstruct's device half (denoise.hip): host arrays in, host arrays out (each optional), blocking, on the current
// device.  `call`: "denoise" with valid == nullptr (out_valid is then not written), "reconstruct" with the "holds a value" byte of every pixel.
int atrous_device(const char* call, uint32_t width, uint32_t height, const double* linear_rgb, const double* variance_rgb, const uint8_t* valid,
                  const double* albedo, const double* normal, const double* depth, const double* alpha, uint32_t iterations, const DenoiseParams& prm,
                  double* out_linear_rgb, uint8_t* out_rgba8, double* out_variance_rgb, uint8_t* out_valid, double* kernel_ms);
// ... and its passes alone, enqueued on `stream` over buffers that are already on the device (the result: d_c[out], d_v[out], d_rgba and, with
// flags, d_out_valid).  d_valid == nullptr: no flags, rttnw_denoise's kernels; d_h (the two ping-pong flag buffers, w*h bytes each) and
// d_out_valid may then be nullptr.
int atrous_passes_device(uint32_t width, uint32_t height, const double* d_in, const double* d_var, const uint8_t* d_valid, const double* d_albedo,
                         const double* d_normal, const double* d_depth, const double* d_alpha, uint32_t iterations, const DenoiseParams& prm,
                         double* const d_c[2], double* const d_v[2], uint8_t* const d_h[2], uint8_t* d_rgba, uint8_t* d_out_valid, hipStream_t stream,
                         int& out);

// rttnw_denoise_nlm's kernels alone (nlm.hip), in the shape of atrous_passes_device: nlm_plan_device picks the filter kernel of the call's radii
// and admits its dynamic LDS — before the caller starts its clock —, nlm_passes_device enqueues the kernels on `stream` over buffers that are
// already on the device: nothing allocated, nothing copied, no wait.  d_var_a / d_var_b: the guides' variances, or both nullptr: the pair
// variance is then formed into d_pair_var (w*h*3).  d_fa / d_fb (w*h*3) take the two cross-filtered halves; d_out, d_err (w*h*3) and d_rgba
// (w*h*4) the mean, the error estimate and the RGBA8 — with d_out == nullptr the finish step is not run.  `at`: the prefix of an error's message.
int nlm_plan_device(const char* at, const NlmParams& prm, NlmPlan& plan);
int nlm_passes_device(const char* at, uint32_t width, uint32_t height, const double* d_a, const double* d_b, const double* d_var_a, const double* d_var_b,
                      double* d_pair_var, const NlmParams& prm, const NlmPlan& plan, double* d_fa, double* d_fb, double* d_out, uint8_t* d_rgba,
                      double* d_err, hipStream_t stream);

// rttnw_denoise_select's device half (select.hip): host arrays in, host arrays out (each optional), blocking, on the current device: two à-trous
// runs, the non-local-means step and the selection (select.hpp) over one set of device buffers.  Arguments were checked by the caller.
int select_device(uint32_t width, uint32_t height, const double* half_a, const double* half_b, const double* var_a, const double* var_b,
                  const double* albedo, const double* normal, const double* depth, const double* alpha, uint32_t iterations, const DenoiseParams& dn,
                  const NlmParams& nl, const SelectParams& sel, double* out_linear_rgb, uint8_t* out_rgba8, double* out_blend, double* out_feature_rgb,
                  double* out_nlm_rgb, double* out_error_rgb, double* kernel_ms);

// rttnw_temporal_accumulate's device half (temporal.hip): host arrays in, host arrays out (each optional), blocking, on the current device: one
// kernel (temporal.hpp).  The prev_* arrays are read only with prm.has_history, the variances only with prm.has_variance.  Arguments were checked
// by the caller.
int temporal_device(uint32_t width, uint32_t height, const TemporalParams& prm, const double* linear_rgb, const double* variance_rgb, const double* normal,
                    const double* depth, const double* alpha, const double* prev_linear_rgb, const double* prev_variance_rgb, const double* prev_length,
                    const double* prev_normal, const double* prev_depth, const double* prev_alpha, double* out_linear_rgb, uint8_t* out_rgba8,
                    double* out_variance_rgb, double* out_length, double* out_prev_xy, double* kernel_ms);

// rttnw_temporal_variance's device half (variance.hip): host arrays in, host arrays out (each optional), blocking, on the current device: the
// accumulation with the second moment, then the estimate (variance.hpp).  The prev_* arrays are read only with prm.has_history.  Arguments were
// checked by the caller.
int variance_device(uint32_t width, uint32_t height, const TemporalParams& prm, const VarianceParams& vprm, const double* linear_rgb, const double* normal,
                    const double* depth, const double* alpha, const double* prev_linear_rgb, const double* prev_moment2_rgb, const double* prev_length,
                    const double* prev_normal, const double* prev_depth, const double* prev_alpha, double* out_linear_rgb, uint8_t* out_rgba8,
                    double* out_moment2_rgb, double* out_length, double* out_prev_xy, double* out_variance_rgb, double* kernel_ms);
// ... and its kernels alone, in the shape of atrous_passes_device: variance_admit_lds admits the estimate kernel's dynamic LDS for a radius — before
// the caller starts its clock —, variance_passes_device enqueues the kernels on `stream` over buffers that are already on the device: nothing
// allocated, nothing copied, no wait.  prm == nullptr: the estimate alone, over a stage A's outputs that d_out, d_m2 and d_len already hold
// (rttnw_svgf_push's accumulate kernel writes them); d_lin, the d_p* buffers, d_rgba and d_xy are then not used.  `at`: the prefix of an error's message.
int variance_admit_lds(const char* at, uint32_t radius);
int variance_passes_device(const char* at, uint32_t width, uint32_t height, const TemporalParams* prm, const VarianceParams& vprm, const double* d_lin,
                           const double* d_normal, const double* d_depth, const double* d_alpha, const double* d_plin, const double* d_pm2,
                           const double* d_plen, const double* d_pnormal, const double* d_pdepth, const double* d_palpha, double* d_out, uint8_t* d_rgba,
                           double* d_m2, double* d_len, double* d_xy, double* d_var, hipStream_t stream);

// rttnw_temporal_clamp's device half (clamp.hip): host arrays in, host arrays out (each optional), blocking, on the current device: the fused
// statistics-and-accumulate kernel of clamp.hpp, then variance.hip's estimate as it is.  Arguments were checked by the caller.
int clamp_device(uint32_t width, uint32_t height, const TemporalParams& prm, const VarianceParams& vprm, const ClampParams& kprm, const double* linear_rgb,
                 const double* normal, const double* depth, const double* alpha, const double* prev_linear_rgb, const double* prev_moment2_rgb,
                 const double* prev_length, const double* prev_normal, const double* prev_depth, const double* prev_alpha, double* out_linear_rgb,
                 uint8_t* out_rgba8, double* out_moment2_rgb, double* out_length, double* out_prev_xy, double* out_variance_rgb, double* out_mean_rgb,
                 double* out_sd_rgb, uint8_t* out_clipped, double* kernel_ms);
// ... and its kernel alone, enqueued on `stream` over buffers that are already on the device: nothing allocated, nothing copied, no wait; its tile
// needs no admission.  With `feedback` the fed-back colour history d_phist rides on the same taps, is clipped into the same interval and blended into
// d_acc (rttnw_svgf_push's step 2); d_clipped (w*h bytes) takes M1's channels in bits 0 - 2 and H's in bits 4 - 6.  d_phist, d_rgba, d_acc, d_mean
// and d_sd may be nullptr.
int clamp_accumulate_device(const char* at, uint32_t width, uint32_t height, const TemporalParams& prm, const ClampParams& kprm, bool feedback,
                            const double* d_lin, const double* d_normal, const double* d_depth, const double* d_alpha, const double* d_pm1, const double* d_pm2,
                            const double* d_phist, const double* d_plen, const double* d_pnormal, const double* d_pdepth, const double* d_palpha, double* d_m1,
                            uint8_t* d_rgba, double* d_m2, double* d_acc, double* d_len, double* d_xy, double* d_mean, double* d_sd, uint8_t* d_clipped,
                            hipStream_t stream);

// rttnw_temporal_probe's device half (probe.hip): host arrays in, host arrays out (each optional), blocking, on the current device: one kernel
// (probe.hpp).  The prev_* arrays are read only with prm.has_history.  Arguments were checked by the caller.
int probe_device(uint32_t width, uint32_t height, const TemporalParams& prm, const SamplingParams& smp, const double* normal, const double* depth,
                 const double* alpha, const double* prev_length, const double* prev_normal, const double* prev_depth, const double* prev_alpha,
                 double* out_length, double* out_prev_xy, uint8_t* out_multiplier, double* kernel_ms);
// ... and what rttnw_svgf_frame enqueues of it on `stream` over buffers that are already on the device: nothing allocated, nothing copied, no wait.
// probe_enqueue_device: the kernel (d_xy may be nullptr); probe_level_mask_device: the byte mask {multiplier == level} over n_pixels pixels, as
// region_select_launch reads one; probe_scatter_device: the selected pixels of a list pass's running sums (n_quads listed blocks, 16 reals of the
// render's precision each) to their places in the packed tiles of a whole frame (tile_world 1).
int probe_enqueue_device(const char* at, uint32_t width, uint32_t height, const TemporalParams& prm, const SamplingParams& smp, const double* d_normal,
                         const double* d_depth, const double* d_alpha, const double* d_plen, const double* d_pnormal, const double* d_pdepth,
                         const double* d_palpha, double* d_len, double* d_xy, uint8_t* d_multiplier, hipStream_t stream);
int probe_level_mask_device(const char* at, uint32_t n_pixels, const uint8_t* d_multiplier, uint32_t level, uint8_t* d_mask, hipStream_t stream);
int probe_scatter_device(const char* at, uint32_t precision, const void* d_sums, const uint32_t* d_quads, uint32_t n_quads, void* d_packed,
                         hipStream_t stream);

// rttnw_denoise's passes with a tap of the pass loop (denoise.hip): atrous_passes_device without flags, and d_tap (w*h*3) receives the linear image
// the same call would return with `tap_after` iterations, 1 <= tap_after <= iterations.  rttnw_svgf_push's feedback.
int atrous_passes_tap_device(uint32_t width, uint32_t height, const double* d_in, const double* d_var, const double* d_albedo, const double* d_normal,
                             const double* d_depth, const double* d_alpha, uint32_t iterations, const DenoiseParams& prm, double* const d_c[2],
                             double* const d_v[2], uint8_t* d_rgba, uint32_t tap_after, double* d_tap, hipStream_t stream, int& out);

} // namespace rt
