// feature_api.cpp — the extern "C" half of rttnw_render_features, rttnw_denoise, rttnw_denoise_nlm, rttnw_denoise_select, rttnw_temporal_accumulate,
// rttnw_temporal_variance and rttnw_reconstruct (include/rttnw_hip.h): argument checks, then the feature pass of the requested arithmetic build (feature_kernels.hpp), the
// device half of the denoiser and of the reconstruction (denoise.hip), the non-local-means filter's (nlm.hip), the per-pixel choice between the two
// (select.hip), the temporal accumulation (temporal.hip), that accumulation with its variance estimate (variance.hip) or with the history clipped to
// the frame in front of it (rttnw_temporal_clamp, clamp.hip), or the colour-free probe of that accumulation (rttnw_temporal_probe, probe.hip); and of
// rttnw_denoise_regress, whose device half (regress.hip) is declared in regress.hpp: no other unit reads it.  Host code only.
#include "feature_api.hpp"
#include "regress.hpp"

namespace rt {

int clamp_refuse_params(const char* call, const rttnw_clamp_params* k) {
    const auto refuse = [call](const char* what) { set_last_error(std::string(call) + ": " + what); return int(RTTNW_ERR_INVALID); };
    if (!k) return refuse("k is NULL");
    if (k->radius > VARIANCE_MAX_RADIUS) return refuse("k->radius is more than 4");
    if (k->reserved0 != 0) return refuse("k->reserved0 must be 0");
    if (!(k->gamma >= 0.0)) return refuse("k->gamma must be >= 0 (and not NaN; +inf never clips)");
    if (!(k->sigma_normal >= 0.0) || !(k->sigma_depth >= 0.0)) return refuse("the sigmas (k->sigma_normal, k->sigma_depth) must be >= 0 (and not NaN)");
    return 0;
}

int sampling_refuse_params(const char* call, const rttnw_sampling_params* a) {
    const auto refuse = [call](const char* what) { set_last_error(std::string(call) + ": " + what); return int(RTTNW_ERR_INVALID); };
    if (!a) return refuse("a is NULL");
    if (a->boost != 0 && a->boost != 1 && a->boost != 2 && a->boost != 4 && a->boost != 8) return refuse("a->boost must be 0 (the default, 8), 1, 2, 4 or 8");
    if (a->reserved0 != 0) return refuse("a->reserved0 must be 0");
    if (!temporal_finite(a->fill) || !(a->fill == 0.0 || a->fill >= 1.0)) return refuse("a->fill must be 0 (the default, 8.0) or finite and >= 1 (and not NaN)");
    return 0;
}

} // namespace rt

extern "C" {

int rttnw_render_features(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, double* out_albedo, double* out_normal,
                          double* out_depth, double* out_alpha, rttnw_stats* stats) {
    // the call's own arguments first, as rttnw_render_adaptive: their refusals need no device (nor a committed scene)
    if (!p) { rt::set_last_error("render_features: NULL argument"); return RTTNW_ERR_INVALID; }
    if (p->spp == 0) { rt::set_last_error("render_features: spp is 0"); return RTTNW_ERR_INVALID; }
    if (int rc = rt::refuse_host_output_misuse("render_features", p->reserved0, p)) return rc;
    if (int rc = rt::validate(s, cam, p)) return rc;
    return RT_BY_PRECISION(p->precision, render_features_t, s, cam, p, out_albedo, out_normal, out_depth, out_alpha, stats);
}

int rttnw_denoise(uint32_t width, uint32_t height, const double* linear_rgb, const double* variance_rgb, const double* albedo, const double* normal,
                  const double* depth, const double* alpha, const rttnw_denoise_params* d, double* out_linear_rgb, uint8_t* out_rgba8,
                  double* out_variance_rgb, double* kernel_ms) {
    if (!linear_rgb || !albedo || !normal || !depth || !alpha || !d) { rt::set_last_error("denoise: NULL argument"); return RTTNW_ERR_INVALID; }
    if (uint64_t(width) * height == 0 || uint64_t(width) * height > (1ull << 28)) { rt::set_last_error("denoise: empty image (or more than 2^28 pixels)"); return RTTNW_ERR_INVALID; }
    if (d->iterations > rt::DENOISE_MAX_ITERATIONS) { rt::set_last_error("denoise: more than 8 iterations"); return RTTNW_ERR_INVALID; }
    if (d->reserved0 != 0) { rt::set_last_error("denoise: reserved0 must be 0"); return RTTNW_ERR_INVALID; }
    if (!(d->sigma_luminance >= 0.0) || !(d->sigma_normal >= 0.0) || !(d->sigma_depth >= 0.0)) {
        rt::set_last_error("denoise: the sigmas must be >= 0 (and not NaN)");
        return RTTNW_ERR_INVALID;
    }
    const rt::DenoiseParams prm = rt::denoise_params(d->sigma_luminance, d->sigma_normal, d->sigma_depth, variance_rgb != nullptr);
    return rt::atrous_device("denoise", width, height, linear_rgb, variance_rgb, nullptr, albedo, normal, depth, alpha, d->iterations, prm, out_linear_rgb,
                             out_rgba8, out_variance_rgb, nullptr, kernel_ms);
}

int rttnw_denoise_nlm(uint32_t width, uint32_t height, const double* half_a, const double* half_b, const double* var_a, const double* var_b,
                      const rttnw_nlm_params* d, double* out_linear_rgb, uint8_t* out_rgba8, double* out_half_a, double* out_half_b, double* out_error_rgb,
                      double* kernel_ms) {
    if (!half_a || !half_b || !d) { rt::set_last_error("denoise_nlm: NULL argument (half_a, half_b or d)"); return RTTNW_ERR_INVALID; }
    if ((var_a == nullptr) != (var_b == nullptr)) { rt::set_last_error("denoise_nlm: var_a and var_b go together: both or neither"); return RTTNW_ERR_INVALID; }
    if (uint64_t(width) * height == 0 || uint64_t(width) * height > (1ull << 28)) {
        rt::set_last_error("denoise_nlm: width * height: empty image (or more than 2^28 pixels)");
        return RTTNW_ERR_INVALID;
    }
    if (d->search_radius > rt::NLM_MAX_SEARCH_RADIUS) { rt::set_last_error("denoise_nlm: d->search_radius is more than 16"); return RTTNW_ERR_INVALID; }
    if (d->patch_radius > rt::NLM_MAX_PATCH_RADIUS) { rt::set_last_error("denoise_nlm: d->patch_radius is more than 4"); return RTTNW_ERR_INVALID; }
    if (d->reserved0 != 0 || d->reserved1 != 0) { rt::set_last_error("denoise_nlm: d->reserved0 and d->reserved1 must be 0"); return RTTNW_ERR_INVALID; }
    if (!(d->k >= 0.0)) { rt::set_last_error("denoise_nlm: d->k must be >= 0 (and not NaN)"); return RTTNW_ERR_INVALID; }
    return rt::nlm_device(width, height, half_a, half_b, var_a, var_b, rt::nlm_params(d->search_radius, d->patch_radius, d->k), out_linear_rgb, out_rgba8,
                          out_half_a, out_half_b, out_error_rgb, kernel_ms);
}

int rttnw_denoise_select(uint32_t width, uint32_t height, const double* half_a, const double* half_b, const double* var_a, const double* var_b,
                         const double* albedo, const double* normal, const double* depth, const double* alpha, const rttnw_denoise_params* dn,
                         const rttnw_nlm_params* nl, const rttnw_select_params* sel, double* out_linear_rgb, uint8_t* out_rgba8, double* out_blend,
                         double* out_feature_rgb, double* out_nlm_rgb, double* out_error_rgb, double* kernel_ms) {
    // what rttnw_denoise_nlm and rttnw_denoise refuse for their own arguments, then the selection's
    const auto refuse = [](const char* what) { rt::set_last_error(std::string("denoise_select: ") + what); return int(RTTNW_ERR_INVALID); };
    if (!half_a || !half_b) return refuse("NULL argument (half_a or half_b)");
    if (!albedo || !normal || !depth || !alpha) return refuse("NULL argument (albedo, normal, depth or alpha)");
    if (!dn || !nl) return refuse("NULL argument (dn or nl)");
    if (!sel) return refuse("sel is NULL");
    if ((var_a == nullptr) != (var_b == nullptr)) return refuse("var_a and var_b go together: both or neither");
    if (uint64_t(width) * height == 0 || uint64_t(width) * height > (1ull << 28)) return refuse("width * height: empty image (or more than 2^28 pixels)");
    if (dn->iterations > rt::DENOISE_MAX_ITERATIONS) return refuse("dn->iterations: more than 8 iterations");
    if (dn->reserved0 != 0) return refuse("dn->reserved0 must be 0");
    if (!(dn->sigma_luminance >= 0.0) || !(dn->sigma_normal >= 0.0) || !(dn->sigma_depth >= 0.0)) {
        return refuse("the sigmas (dn->sigma_luminance, sigma_normal, sigma_depth) must be >= 0 (and not NaN)");
    }
    if (nl->search_radius > rt::NLM_MAX_SEARCH_RADIUS) return refuse("nl->search_radius is more than 16");
    if (nl->patch_radius > rt::NLM_MAX_PATCH_RADIUS) return refuse("nl->patch_radius is more than 4");
    if (nl->reserved0 != 0 || nl->reserved1 != 0) return refuse("nl->reserved0 and nl->reserved1 must be 0");
    if (!(nl->k >= 0.0)) return refuse("nl->k must be >= 0 (and not NaN)");
    if (sel->error_radius > rt::SELECT_MAX_ERROR_RADIUS) return refuse("sel->error_radius is more than 16");
    if (sel->blend_radius > rt::SELECT_MAX_BLEND_RADIUS) return refuse("sel->blend_radius is more than 8");
    if (sel->reserved0 != 0) return refuse("sel->reserved0 must be 0");
    if (sel->use_default_margin == 0 && !(sel->margin >= -2.0 && sel->margin <= 2.0)) return refuse("sel->margin must lie in [-2, 2] (and not be NaN)");
    return rt::select_device(width, height, half_a, half_b, var_a, var_b, albedo, normal, depth, alpha, dn->iterations,
                             rt::denoise_params(dn->sigma_luminance, dn->sigma_normal, dn->sigma_depth, var_a != nullptr),
                             rt::nlm_params(nl->search_radius, nl->patch_radius, nl->k),
                             rt::select_params(sel->error_radius, sel->blend_radius, sel->margin, sel->use_default_margin != 0), out_linear_rgb, out_rgba8,
                             out_blend, out_feature_rgb, out_nlm_rgb, out_error_rgb, kernel_ms);
}

int rttnw_denoise_regress(uint32_t width, uint32_t height, const double* half_a, const double* half_b, const double* var_a, const double* var_b,
                          const double* albedo, const double* normal, const double* depth, const double* alpha, const rttnw_regress_params* g,
                          double* out_linear_rgb, uint8_t* out_rgba8, double* out_half_a, double* out_half_b, double* out_error_rgb, double* out_fit,
                          double* kernel_ms) {
    // what rttnw_denoise_nlm refuses for the arguments the two share, in its order, then the regression's own, in the struct's order
    const auto refuse = [](const char* what) { rt::set_last_error(std::string("denoise_regress: ") + what); return int(RTTNW_ERR_INVALID); };
    if (!half_a || !half_b) return refuse("NULL argument (half_a or half_b)");
    if (!g) return refuse("g is NULL");
    if ((var_a == nullptr) != (var_b == nullptr)) return refuse("var_a and var_b go together: both or neither");
    if (uint64_t(width) * height == 0 || uint64_t(width) * height > (1ull << 28)) return refuse("width * height: empty image (or more than 2^28 pixels)");
    if (g->search_radius > rt::NLM_MAX_SEARCH_RADIUS) return refuse("g->search_radius is more than 16");
    if (g->patch_radius > rt::NLM_MAX_PATCH_RADIUS) return refuse("g->patch_radius is more than 4");
    if (!(g->k >= 0.0)) return refuse("g->k must be >= 0 (and not NaN)");
    if (g->features > rt::REGRESS_ALL) return refuse("g->features is more than 7 (bits: 1 albedo, 2 normal, 4 depth)");
    if (!(g->ridge >= 0.0)) return refuse("g->ridge must be >= 0 (and not NaN)");
    if (g->reserved0 != 0 || g->reserved1 != 0) return refuse("g->reserved0 and g->reserved1 must be 0");
    if (g->features != 0 && !alpha) return refuse("alpha is NULL: g->features != 0 needs it");
    if ((g->features & rt::REGRESS_ALBEDO) && !albedo) return refuse("albedo is NULL: bit 1 of g->features selects it");
    if ((g->features & rt::REGRESS_NORMAL) && !normal) return refuse("normal is NULL: bit 2 of g->features selects it");
    if ((g->features & rt::REGRESS_DEPTH) && !depth) return refuse("depth is NULL: bit 4 of g->features selects it");
    if (g->demodulate != 0 && (!albedo || !alpha)) return refuse("g->demodulate != 0 needs albedo and alpha");
    return rt::regress_device(width, height, half_a, half_b, var_a, var_b, albedo, normal, depth, alpha,
                              rt::regress_params(g->search_radius, g->patch_radius, g->k, g->ridge, g->features, g->demodulate), out_linear_rgb,
                              out_rgba8, out_half_a, out_half_b, out_error_rgb, out_fit, kernel_ms);
}

int rttnw_temporal_accumulate(uint32_t width, uint32_t height, const rttnw_camera_desc* cam, const rttnw_camera_desc* prev_cam, const double* linear_rgb,
                              const double* variance_rgb, const double* normal, const double* depth, const double* alpha, const double* prev_linear_rgb,
                              const double* prev_variance_rgb, const double* prev_length, const double* prev_normal, const double* prev_depth,
                              const double* prev_alpha, const rttnw_temporal_params* t, double* out_linear_rgb, uint8_t* out_rgba8, double* out_variance_rgb,
                              double* out_length, double* out_prev_xy, double* kernel_ms) {
    const auto refuse = [](const char* what) { rt::set_last_error(std::string("temporal_accumulate: ") + what); return int(RTTNW_ERR_INVALID); };
    if (!cam) return refuse("cam is NULL");
    if (!linear_rgb) return refuse("linear_rgb is NULL");
    if (!normal || !depth || !alpha) return refuse("NULL argument (normal, depth or alpha)");
    if (!t) return refuse("t is NULL");
    if (uint64_t(width) * height == 0 || uint64_t(width) * height > (1ull << 28)) return refuse("width * height: empty image (or more than 2^28 pixels)");
    // the history: the previous frame's accumulated colour and length and its feature maps; its variances go with this frame's
    const int given = (prev_linear_rgb != nullptr) + (prev_length != nullptr) + (prev_normal != nullptr) + (prev_depth != nullptr) + (prev_alpha != nullptr);
    const bool has_history = given == 5;
    if ((given != 0 && given != 5) || (given == 0 && prev_variance_rgb)) {
        return refuse("the prev_* arrays go together: prev_linear_rgb, prev_length, prev_normal, prev_depth and prev_alpha all, or none of the six");
    }
    if (has_history && !prev_cam) return refuse("prev_cam is NULL beside a history");
    if (has_history && (variance_rgb == nullptr) != (prev_variance_rgb == nullptr)) {
        return refuse("variance_rgb and prev_variance_rgb go together beside a history: both or neither");
    }
    if (t->max_history > rt::TEMPORAL_HISTORY_LIMIT) return refuse("t->max_history is more than 65535");
    if (t->reserved0 != 0) return refuse("t->reserved0 must be 0");
    if (!(t->depth_tolerance >= 0.0)) return refuse("t->depth_tolerance must be >= 0 (and not NaN)");
    if (!(t->normal_min >= -1.0 && t->normal_min <= 1.0)) return refuse("t->normal_min must lie in [-1, 1] (and not be NaN)");
    const rt::CameraRec<double> rec = rt::camera_of<double>(cam);
    rt::CameraRec<double> prev_rec = {};
    if (has_history) prev_rec = rt::camera_of<double>(prev_cam);
    const bool same_camera = has_history && std::memcmp(cam, prev_cam, sizeof(rttnw_camera_desc)) == 0;
    const rt::TemporalParams prm = rt::temporal_params(rec, has_history ? &prev_rec : nullptr, same_camera, t->max_history, t->depth_tolerance, t->normal_min,
                                                       variance_rgb != nullptr);
    return rt::temporal_device(width, height, prm, linear_rgb, variance_rgb, normal, depth, alpha, prev_linear_rgb, prev_variance_rgb, prev_length, prev_normal,
                               prev_depth, prev_alpha, out_linear_rgb, out_rgba8, out_variance_rgb, out_length, out_prev_xy, kernel_ms);
}

int rttnw_temporal_variance(uint32_t width, uint32_t height, const rttnw_camera_desc* cam, const rttnw_camera_desc* prev_cam, const double* linear_rgb,
                            const double* normal, const double* depth, const double* alpha, const double* prev_linear_rgb, const double* prev_moment2_rgb,
                            const double* prev_length, const double* prev_normal, const double* prev_depth, const double* prev_alpha,
                            const rttnw_temporal_params* t, const rttnw_variance_params* v, double* out_linear_rgb, uint8_t* out_rgba8,
                            double* out_moment2_rgb, double* out_length, double* out_prev_xy, double* out_variance_rgb, double* kernel_ms) {
    // what rttnw_temporal_accumulate refuses for the arguments the two share, then the estimate's own
    const auto refuse = [](const char* what) { rt::set_last_error(std::string("temporal_variance: ") + what); return int(RTTNW_ERR_INVALID); };
    if (!cam) return refuse("cam is NULL");
    if (!linear_rgb) return refuse("linear_rgb is NULL");
    if (!normal || !depth || !alpha) return refuse("NULL argument (normal, depth or alpha)");
    if (!t) return refuse("t is NULL");
    if (uint64_t(width) * height == 0 || uint64_t(width) * height > (1ull << 28)) return refuse("width * height: empty image (or more than 2^28 pixels)");
    const int given = (prev_linear_rgb != nullptr) + (prev_moment2_rgb != nullptr) + (prev_length != nullptr) + (prev_normal != nullptr) +
                      (prev_depth != nullptr) + (prev_alpha != nullptr);
    const bool has_history = given == 6;
    if (given != 0 && given != 6) {
        return refuse("the prev_* arrays go together: prev_linear_rgb, prev_moment2_rgb, prev_length, prev_normal, prev_depth and prev_alpha all, or none");
    }
    if (has_history && !prev_cam) return refuse("prev_cam is NULL beside a history");
    if (t->max_history > rt::TEMPORAL_HISTORY_LIMIT) return refuse("t->max_history is more than 65535");
    if (t->reserved0 != 0) return refuse("t->reserved0 must be 0");
    if (!(t->depth_tolerance >= 0.0)) return refuse("t->depth_tolerance must be >= 0 (and not NaN)");
    if (!(t->normal_min >= -1.0 && t->normal_min <= 1.0)) return refuse("t->normal_min must lie in [-1, 1] (and not be NaN)");
    if (!v) return refuse("v is NULL");
    if (v->min_temporal == 1 || v->min_temporal > rt::TEMPORAL_HISTORY_LIMIT) return refuse("v->min_temporal must be 0 (the default, 4) or 2 .. 65535");
    if (v->radius > rt::VARIANCE_MAX_RADIUS) return refuse("v->radius is more than 4");
    if (v->reserved0 != 0 || v->reserved1 != 0) return refuse("v->reserved0 and v->reserved1 must be 0");
    if (!(v->sigma_normal >= 0.0) || !(v->sigma_depth >= 0.0)) return refuse("the sigmas (v->sigma_normal, v->sigma_depth) must be >= 0 (and not NaN)");
    const rt::CameraRec<double> rec = rt::camera_of<double>(cam);
    rt::CameraRec<double> prev_rec = {};
    if (has_history) prev_rec = rt::camera_of<double>(prev_cam);
    const bool same_camera = has_history && std::memcmp(cam, prev_cam, sizeof(rttnw_camera_desc)) == 0;
    const rt::TemporalParams prm = rt::temporal_params(rec, has_history ? &prev_rec : nullptr, same_camera, t->max_history, t->depth_tolerance, t->normal_min, false);
    return rt::variance_device(width, height, prm, rt::variance_params(v->min_temporal, v->radius, v->sigma_normal, v->sigma_depth), linear_rgb, normal, depth,
                               alpha, prev_linear_rgb, prev_moment2_rgb, prev_length, prev_normal, prev_depth, prev_alpha, out_linear_rgb, out_rgba8,
                               out_moment2_rgb, out_length, out_prev_xy, out_variance_rgb, kernel_ms);
}

int rttnw_temporal_clamp(uint32_t width, uint32_t height, const rttnw_camera_desc* cam, const rttnw_camera_desc* prev_cam, const double* linear_rgb,
                         const double* normal, const double* depth, const double* alpha, const double* prev_linear_rgb, const double* prev_moment2_rgb,
                         const double* prev_length, const double* prev_normal, const double* prev_depth, const double* prev_alpha,
                         const rttnw_temporal_params* t, const rttnw_variance_params* v, const rttnw_clamp_params* k, double* out_linear_rgb,
                         uint8_t* out_rgba8, double* out_moment2_rgb, double* out_length, double* out_prev_xy, double* out_variance_rgb, double* out_mean_rgb,
                         double* out_sd_rgb, uint8_t* out_clipped, double* kernel_ms) {
    // what rttnw_temporal_variance refuses, in its order, then the clip's own
    const auto refuse = [](const char* what) { rt::set_last_error(std::string("temporal_clamp: ") + what); return int(RTTNW_ERR_INVALID); };
    if (!cam) return refuse("cam is NULL");
    if (!linear_rgb) return refuse("linear_rgb is NULL");
    if (!normal || !depth || !alpha) return refuse("NULL argument (normal, depth or alpha)");
    if (!t) return refuse("t is NULL");
    if (uint64_t(width) * height == 0 || uint64_t(width) * height > (1ull << 28)) return refuse("width * height: empty image (or more than 2^28 pixels)");
    const int given = (prev_linear_rgb != nullptr) + (prev_moment2_rgb != nullptr) + (prev_length != nullptr) + (prev_normal != nullptr) +
                      (prev_depth != nullptr) + (prev_alpha != nullptr);
    const bool has_history = given == 6;
    if (given != 0 && given != 6) {
        return refuse("the prev_* arrays go together: prev_linear_rgb, prev_moment2_rgb, prev_length, prev_normal, prev_depth and prev_alpha all, or none");
    }
    if (has_history && !prev_cam) return refuse("prev_cam is NULL beside a history");
    if (t->max_history > rt::TEMPORAL_HISTORY_LIMIT) return refuse("t->max_history is more than 65535");
    if (t->reserved0 != 0) return refuse("t->reserved0 must be 0");
    if (!(t->depth_tolerance >= 0.0)) return refuse("t->depth_tolerance must be >= 0 (and not NaN)");
    if (!(t->normal_min >= -1.0 && t->normal_min <= 1.0)) return refuse("t->normal_min must lie in [-1, 1] (and not be NaN)");
    if (!v) return refuse("v is NULL");
    if (v->min_temporal == 1 || v->min_temporal > rt::TEMPORAL_HISTORY_LIMIT) return refuse("v->min_temporal must be 0 (the default, 4) or 2 .. 65535");
    if (v->radius > rt::VARIANCE_MAX_RADIUS) return refuse("v->radius is more than 4");
    if (v->reserved0 != 0 || v->reserved1 != 0) return refuse("v->reserved0 and v->reserved1 must be 0");
    if (!(v->sigma_normal >= 0.0) || !(v->sigma_depth >= 0.0)) return refuse("the sigmas (v->sigma_normal, v->sigma_depth) must be >= 0 (and not NaN)");
    if (int rc = rt::clamp_refuse_params("temporal_clamp", k)) return rc;
    const rt::CameraRec<double> rec = rt::camera_of<double>(cam);
    rt::CameraRec<double> prev_rec = {};
    if (has_history) prev_rec = rt::camera_of<double>(prev_cam);
    const bool same_camera = has_history && std::memcmp(cam, prev_cam, sizeof(rttnw_camera_desc)) == 0;
    const rt::TemporalParams prm = rt::temporal_params(rec, has_history ? &prev_rec : nullptr, same_camera, t->max_history, t->depth_tolerance, t->normal_min, false);
    return rt::clamp_device(width, height, prm, rt::variance_params(v->min_temporal, v->radius, v->sigma_normal, v->sigma_depth),
                            rt::clamp_params(k->radius, k->gamma, k->sigma_normal, k->sigma_depth), linear_rgb, normal, depth, alpha, prev_linear_rgb,
                            prev_moment2_rgb, prev_length, prev_normal, prev_depth, prev_alpha, out_linear_rgb, out_rgba8, out_moment2_rgb, out_length,
                            out_prev_xy, out_variance_rgb, out_mean_rgb, out_sd_rgb, out_clipped, kernel_ms);
}

int rttnw_temporal_probe(uint32_t width, uint32_t height, const rttnw_camera_desc* cam, const rttnw_camera_desc* prev_cam, const double* normal,
                         const double* depth, const double* alpha, const double* prev_length, const double* prev_normal, const double* prev_depth,
                         const double* prev_alpha, const rttnw_temporal_params* t, const rttnw_sampling_params* a, double* out_length, double* out_prev_xy,
                         uint8_t* out_multiplier, double* kernel_ms) {
    // what rttnw_temporal_accumulate refuses for the arguments the two share, in its order, then the sampling block's own
    const auto refuse = [](const char* what) { rt::set_last_error(std::string("temporal_probe: ") + what); return int(RTTNW_ERR_INVALID); };
    if (!cam) return refuse("cam is NULL");
    if (!normal || !depth || !alpha) return refuse("NULL argument (normal, depth or alpha)");
    if (!t) return refuse("t is NULL");
    if (uint64_t(width) * height == 0 || uint64_t(width) * height > (1ull << 28)) return refuse("width * height: empty image (or more than 2^28 pixels)");
    const int given = (prev_length != nullptr) + (prev_normal != nullptr) + (prev_depth != nullptr) + (prev_alpha != nullptr);
    const bool has_history = given == 4;
    if (given != 0 && given != 4) return refuse("the prev_* arrays go together: prev_length, prev_normal, prev_depth and prev_alpha all, or none");
    if (has_history && !prev_cam) return refuse("prev_cam is NULL beside a history");
    if (t->max_history > rt::TEMPORAL_HISTORY_LIMIT) return refuse("t->max_history is more than 65535");
    if (t->reserved0 != 0) return refuse("t->reserved0 must be 0");
    if (!(t->depth_tolerance >= 0.0)) return refuse("t->depth_tolerance must be >= 0 (and not NaN)");
    if (!(t->normal_min >= -1.0 && t->normal_min <= 1.0)) return refuse("t->normal_min must lie in [-1, 1] (and not be NaN)");
    if (int rc = rt::sampling_refuse_params("temporal_probe", a)) return rc;
    const rt::CameraRec<double> rec = rt::camera_of<double>(cam);
    rt::CameraRec<double> prev_rec = {};
    if (has_history) prev_rec = rt::camera_of<double>(prev_cam);
    const bool same_camera = has_history && std::memcmp(cam, prev_cam, sizeof(rttnw_camera_desc)) == 0;
    const rt::TemporalParams prm = rt::temporal_params(rec, has_history ? &prev_rec : nullptr, same_camera, t->max_history, t->depth_tolerance, t->normal_min, false);
    return rt::probe_device(width, height, prm, rt::sampling_params(a->boost, a->fill), normal, depth, alpha, prev_length, prev_normal, prev_depth, prev_alpha,
                            out_length, out_prev_xy, out_multiplier, kernel_ms);
}

int rttnw_reconstruct(uint32_t width, uint32_t height, const double* linear_rgb, const double* variance_rgb, const uint8_t* valid, const double* albedo,
                      const double* normal, const double* depth, const double* alpha, const rttnw_denoise_params* d, double* out_linear_rgb,
                      uint8_t* out_rgba8, double* out_variance_rgb, uint8_t* out_valid, double* kernel_ms) {
    // rttnw_denoise's refusals, with its codes, and the flags'
    if (!linear_rgb || !albedo || !normal || !depth || !alpha || !d) {
        rt::set_last_error("reconstruct: NULL argument (linear_rgb, albedo, normal, depth, alpha or d)");
        return RTTNW_ERR_INVALID;
    }
    if (!valid) { rt::set_last_error("reconstruct: valid is NULL"); return RTTNW_ERR_INVALID; }
    if (uint64_t(width) * height == 0 || uint64_t(width) * height > (1ull << 28)) {
        rt::set_last_error("reconstruct: width * height: empty image (or more than 2^28 pixels)");
        return RTTNW_ERR_INVALID;
    }
    if (d->iterations > rt::DENOISE_MAX_ITERATIONS) { rt::set_last_error("reconstruct: d->iterations: more than 8 iterations"); return RTTNW_ERR_INVALID; }
    if (d->reserved0 != 0) { rt::set_last_error("reconstruct: d->reserved0 must be 0"); return RTTNW_ERR_INVALID; }
    if (!(d->sigma_luminance >= 0.0) || !(d->sigma_normal >= 0.0) || !(d->sigma_depth >= 0.0)) {
        rt::set_last_error("reconstruct: the sigmas (sigma_luminance, sigma_normal, sigma_depth) must be >= 0 (and not NaN)");
        return RTTNW_ERR_INVALID;
    }
    const rt::DenoiseParams prm = rt::denoise_params(d->sigma_luminance, d->sigma_normal, d->sigma_depth, variance_rgb != nullptr);
    return rt::atrous_device("reconstruct", width, height, linear_rgb, variance_rgb, valid, albedo, normal, depth, alpha, d->iterations, prm, out_linear_rgb,
                             out_rgba8, out_variance_rgb, out_valid, kernel_ms);
}

} // extern "C"
