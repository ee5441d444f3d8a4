// feature_api.cpp — the extern "C" half of rttnw_render_features and of the nine image-filter entry points (include/rttnw_hip.h): rttnw_denoise and
// rttnw_reconstruct (device half: denoise.hip), rttnw_denoise_nlm (nlm.hip), rttnw_denoise_select (select.hip), rttnw_denoise_regress (regress.hip,
// declared in regress.hpp: no other unit reads it), rttnw_temporal_accumulate (temporal.hip), rttnw_temporal_variance (variance.hip),
// rttnw_temporal_clamp (clamp.hip) and rttnw_temporal_probe (probe.hip).  Each checks its arguments — one refusal function per parameter block,
// below, which svgf.hip and render_adaptive_api.cpp call for the same blocks inside their own structs — and hands them to the device half.
// Host code only.
#include "feature_api.hpp"
#include "regress.hpp"

namespace rt {

int refuse(const char* call, const std::string& what) {
    set_last_error(std::string(call) + ": " + what);
    return RTTNW_ERR_INVALID;
}

int image_size_refused(const char* call, uint32_t width, uint32_t height) {
    const uint64_t npx = uint64_t(width) * height;
    if (npx == 0 || npx > (1ull << 28)) return refuse(call,"width * height: empty image (or more than 2^28 pixels)");
    return 0;
}

int temporal_refuse_params(const char* call, const char* field, const rttnw_temporal_params& t) {
    const std::string f(field);
    if (t.max_history > TEMPORAL_HISTORY_LIMIT) return refuse(call,f + "max_history is more than 65535");
    if (t.reserved0 != 0) return refuse(call,f + "reserved0 must be 0");
    if (!(t.depth_tolerance >= 0.0)) return refuse(call,f + "depth_tolerance must be >= 0 (and not NaN)");
    if (!(t.normal_min >= -1.0 && t.normal_min <= 1.0)) return refuse(call,f + "normal_min must lie in [-1, 1] (and not be NaN)");
    return 0;
}

int variance_refuse_params(const char* call, const char* field, const rttnw_variance_params& v) {
    const std::string f(field);
    if (v.min_temporal == 1 || v.min_temporal > TEMPORAL_HISTORY_LIMIT) return refuse(call,f + "min_temporal must be 0 (the default, 4) or 2 .. 65535");
    if (v.radius > VARIANCE_MAX_RADIUS) return refuse(call,f + "radius is more than 4");
    if (v.reserved0 != 0 || v.reserved1 != 0) return refuse(call,f + "reserved0 and " + f + "reserved1 must be 0");
    if (!(v.sigma_normal >= 0.0) || !(v.sigma_depth >= 0.0)) {
        return refuse(call,"the sigmas (" + f + "sigma_normal, " + f + "sigma_depth) must be >= 0 (and not NaN)");
    }
    return 0;
}

int denoise_refuse_params(const char* call, const char* field, const rttnw_denoise_params& d) {
    const std::string f(field);
    if (d.iterations > DENOISE_MAX_ITERATIONS) return refuse(call,f + "iterations: more than 8 iterations");
    if (d.reserved0 != 0) return refuse(call,f + "reserved0 must be 0");
    if (!(d.sigma_luminance >= 0.0) || !(d.sigma_normal >= 0.0) || !(d.sigma_depth >= 0.0)) {
        return refuse(call,"the sigmas (" + f + "sigma_luminance, sigma_normal, sigma_depth) must be >= 0 (and not NaN)");
    }
    return 0;
}

int nlm_refuse_params(const char* call, const char* field, const rttnw_nlm_params& d) {
    const std::string f(field);
    if (d.search_radius > NLM_MAX_SEARCH_RADIUS) return refuse(call,f + "search_radius is more than 16");
    if (d.patch_radius > NLM_MAX_PATCH_RADIUS) return refuse(call,f + "patch_radius is more than 4");
    if (d.reserved0 != 0 || d.reserved1 != 0) return refuse(call,f + "reserved0 and " + f + "reserved1 must be 0");
    if (!(d.k >= 0.0)) return refuse(call,f + "k must be >= 0 (and not NaN)");
    return 0;
}

int regress_refuse_params(const char* call, const rttnw_regress_params* g) {
    if (!g) return refuse(call, "g is NULL");
    if (g->search_radius > NLM_MAX_SEARCH_RADIUS) return refuse(call, "g->search_radius is more than 16");
    if (g->patch_radius > NLM_MAX_PATCH_RADIUS) return refuse(call, "g->patch_radius is more than 4");
    if (!(g->k >= 0.0)) return refuse(call, "g->k must be >= 0 (and not NaN)");
    if (g->features > REGRESS_ALL) return refuse(call, "g->features is more than 7 (bits: 1 albedo, 2 normal, 4 depth)");
    if (!(g->ridge >= 0.0)) return refuse(call, "g->ridge must be >= 0 (and not NaN)");
    if (g->reserved0 != 0 || g->reserved1 != 0) return refuse(call, "g->reserved0 and g->reserved1 must be 0");
    return 0;
}

int clamp_refuse_params(const char* call, const rttnw_clamp_params* k) {
    if (!k) return refuse(call,"k is NULL");
    if (k->radius > VARIANCE_MAX_RADIUS) return refuse(call,"k->radius is more than 4");
    if (k->reserved0 != 0) return refuse(call,"k->reserved0 must be 0");
    if (!(k->gamma >= 0.0)) return refuse(call,"k->gamma must be >= 0 (and not NaN; +inf never clips)");
    if (!(k->sigma_normal >= 0.0) || !(k->sigma_depth >= 0.0)) return refuse(call,"the sigmas (k->sigma_normal, k->sigma_depth) must be >= 0 (and not NaN)");
    return 0;
}

int sampling_refuse_params(const char* call, const rttnw_sampling_params* a) {
    if (!a) return refuse(call,"a is NULL");
    if (a->boost != 0 && a->boost != 1 && a->boost != 2 && a->boost != 4 && a->boost != 8) return refuse(call,"a->boost must be 0 (the default, 8), 1, 2, 4 or 8");
    if (a->reserved0 != 0) return refuse(call,"a->reserved0 must be 0");
    if (!temporal_finite(a->fill) || !(a->fill == 0.0 || a->fill >= 1.0)) return refuse(call,"a->fill must be 0 (the default, 8.0) or finite and >= 1 (and not NaN)");
    return 0;
}

TemporalParams history_temporal_params(const rttnw_camera_desc* cam, const rttnw_camera_desc* prev_cam, const rttnw_temporal_params& t, bool has_variance) {
    const CameraRec<double> rec = camera_of<double>(cam);
    CameraRec<double> prev_rec = {};
    if (prev_cam) prev_rec = camera_of<double>(prev_cam);
    const bool same_camera = prev_cam && std::memcmp(cam, prev_cam, sizeof(rttnw_camera_desc)) == 0;
    return temporal_params(rec, prev_cam ? &prev_rec : nullptr, same_camera, t.max_history, t.depth_tolerance, t.normal_min, has_variance);
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
    const char* const call = "denoise";
    if (!linear_rgb || !albedo || !normal || !depth || !alpha || !d) return rt::refuse(call, "NULL argument");
    if (int rc = rt::image_size_refused(call, width, height)) return rc;
    if (int rc = rt::denoise_refuse_params(call, "d->", *d)) return rc;
    const rt::DenoiseParams prm = rt::denoise_params(d->sigma_luminance, d->sigma_normal, d->sigma_depth, variance_rgb != nullptr);
    return rt::atrous_device(call, width, height, linear_rgb, variance_rgb, nullptr, albedo, normal, depth, alpha, d->iterations, prm, out_linear_rgb,
                             out_rgba8, out_variance_rgb, nullptr, kernel_ms);
}

int rttnw_denoise_nlm(uint32_t width, uint32_t height, const double* half_a, const double* half_b, const double* var_a, const double* var_b,
                      const rttnw_nlm_params* d, double* out_linear_rgb, uint8_t* out_rgba8, double* out_half_a, double* out_half_b, double* out_error_rgb,
                      double* kernel_ms) {
    const char* const call = "denoise_nlm";
    if (!half_a || !half_b || !d) return rt::refuse(call, "NULL argument (half_a, half_b or d)");
    if ((var_a == nullptr) != (var_b == nullptr)) return rt::refuse(call, "var_a and var_b go together: both or neither");
    if (int rc = rt::image_size_refused(call, width, height)) return rc;
    if (int rc = rt::nlm_refuse_params(call, "d->", *d)) return rc;
    return rt::nlm_device(width, height, half_a, half_b, var_a, var_b, rt::nlm_params(d->search_radius, d->patch_radius, d->k), out_linear_rgb, out_rgba8,
                          out_half_a, out_half_b, out_error_rgb, kernel_ms);
}

int rttnw_denoise_select(uint32_t width, uint32_t height, const double* half_a, const double* half_b, const double* var_a, const double* var_b,
                         const double* albedo, const double* normal, const double* depth, const double* alpha, const rttnw_denoise_params* dn,
                         const rttnw_nlm_params* nl, const rttnw_select_params* sel, double* out_linear_rgb, uint8_t* out_rgba8, double* out_blend,
                         double* out_feature_rgb, double* out_nlm_rgb, double* out_error_rgb, double* kernel_ms) {
    // what rttnw_denoise_nlm and rttnw_denoise refuse for their own arguments, then the selection's
    const char* const call = "denoise_select";
    if (!half_a || !half_b) return rt::refuse(call, "NULL argument (half_a or half_b)");
    if (!albedo || !normal || !depth || !alpha) return rt::refuse(call, "NULL argument (albedo, normal, depth or alpha)");
    if (!dn || !nl) return rt::refuse(call, "NULL argument (dn or nl)");
    if (!sel) return rt::refuse(call, "sel is NULL");
    if ((var_a == nullptr) != (var_b == nullptr)) return rt::refuse(call, "var_a and var_b go together: both or neither");
    if (int rc = rt::image_size_refused(call, width, height)) return rc;
    if (int rc = rt::denoise_refuse_params(call, "dn->", *dn)) return rc;
    if (int rc = rt::nlm_refuse_params(call, "nl->", *nl)) return rc;
    if (sel->error_radius > rt::SELECT_MAX_ERROR_RADIUS) return rt::refuse(call, "sel->error_radius is more than 16");
    if (sel->blend_radius > rt::SELECT_MAX_BLEND_RADIUS) return rt::refuse(call, "sel->blend_radius is more than 8");
    if (sel->reserved0 != 0) return rt::refuse(call, "sel->reserved0 must be 0");
    if (sel->use_default_margin == 0 && !(sel->margin >= -2.0 && sel->margin <= 2.0)) return rt::refuse(call, "sel->margin must lie in [-2, 2] (and not be NaN)");
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
    const char* const call = "denoise_regress";
    if (!half_a || !half_b) return rt::refuse(call, "NULL argument (half_a or half_b)");
    if (!g) return rt::refuse(call, "g is NULL");
    if ((var_a == nullptr) != (var_b == nullptr)) return rt::refuse(call, "var_a and var_b go together: both or neither");
    if (int rc = rt::image_size_refused(call, width, height)) return rc;
    if (int rc = rt::regress_refuse_params(call, g)) return rc;
    if (g->features != 0 && !alpha) return rt::refuse(call, "alpha is NULL: g->features != 0 needs it");
    if ((g->features & rt::REGRESS_ALBEDO) && !albedo) return rt::refuse(call, "albedo is NULL: bit 1 of g->features selects it");
    if ((g->features & rt::REGRESS_NORMAL) && !normal) return rt::refuse(call, "normal is NULL: bit 2 of g->features selects it");
    if ((g->features & rt::REGRESS_DEPTH) && !depth) return rt::refuse(call, "depth is NULL: bit 4 of g->features selects it");
    if (g->demodulate != 0 && (!albedo || !alpha)) return rt::refuse(call, "g->demodulate != 0 needs albedo and alpha");
    return rt::regress_device(width, height, half_a, half_b, var_a, var_b, albedo, normal, depth, alpha,
                              rt::regress_params(g->search_radius, g->patch_radius, g->k, g->ridge, g->features, g->demodulate), out_linear_rgb,
                              out_rgba8, out_half_a, out_half_b, out_error_rgb, out_fit, kernel_ms);
}

int rttnw_temporal_accumulate(uint32_t width, uint32_t height, const rttnw_camera_desc* cam, const rttnw_camera_desc* prev_cam, const double* linear_rgb,
                              const double* variance_rgb, const double* normal, const double* depth, const double* alpha, const double* prev_linear_rgb,
                              const double* prev_variance_rgb, const double* prev_length, const double* prev_normal, const double* prev_depth,
                              const double* prev_alpha, const rttnw_temporal_params* t, double* out_linear_rgb, uint8_t* out_rgba8, double* out_variance_rgb,
                              double* out_length, double* out_prev_xy, double* kernel_ms) {
    const char* const call = "temporal_accumulate";
    if (!cam) return rt::refuse(call, "cam is NULL");
    if (!linear_rgb) return rt::refuse(call, "linear_rgb is NULL");
    if (!normal || !depth || !alpha) return rt::refuse(call, "NULL argument (normal, depth or alpha)");
    if (!t) return rt::refuse(call, "t is NULL");
    if (int rc = rt::image_size_refused(call, width, height)) return rc;
    // the history: the previous frame's accumulated colour and length and its feature maps; its variances go with this frame's
    const int given = (prev_linear_rgb != nullptr) + (prev_length != nullptr) + (prev_normal != nullptr) + (prev_depth != nullptr) + (prev_alpha != nullptr);
    const bool has_history = given == 5;
    if ((given != 0 && given != 5) || (given == 0 && prev_variance_rgb)) {
        return rt::refuse(call, "the prev_* arrays go together: prev_linear_rgb, prev_length, prev_normal, prev_depth and prev_alpha all, or none of the six");
    }
    if (has_history && !prev_cam) return rt::refuse(call, "prev_cam is NULL beside a history");
    if (has_history && (variance_rgb == nullptr) != (prev_variance_rgb == nullptr)) {
        return rt::refuse(call, "variance_rgb and prev_variance_rgb go together beside a history: both or neither");
    }
    if (int rc = rt::temporal_refuse_params(call, "t->", *t)) return rc;
    const rt::TemporalParams prm = rt::history_temporal_params(cam, has_history ? prev_cam : nullptr, *t, variance_rgb != nullptr);
    return rt::temporal_device(width, height, prm, linear_rgb, variance_rgb, normal, depth, alpha, prev_linear_rgb, prev_variance_rgb, prev_length, prev_normal,
                               prev_depth, prev_alpha, out_linear_rgb, out_rgba8, out_variance_rgb, out_length, out_prev_xy, kernel_ms);
}

int rttnw_temporal_variance(uint32_t width, uint32_t height, const rttnw_camera_desc* cam, const rttnw_camera_desc* prev_cam, const double* linear_rgb,
                            const double* normal, const double* depth, const double* alpha, const double* prev_linear_rgb, const double* prev_moment2_rgb,
                            const double* prev_length, const double* prev_normal, const double* prev_depth, const double* prev_alpha,
                            const rttnw_temporal_params* t, const rttnw_variance_params* v, double* out_linear_rgb, uint8_t* out_rgba8,
                            double* out_moment2_rgb, double* out_length, double* out_prev_xy, double* out_variance_rgb, double* kernel_ms) {
    // what rttnw_temporal_accumulate refuses for the arguments the two share, then the estimate's own
    const char* const call = "temporal_variance";
    if (!cam) return rt::refuse(call, "cam is NULL");
    if (!linear_rgb) return rt::refuse(call, "linear_rgb is NULL");
    if (!normal || !depth || !alpha) return rt::refuse(call, "NULL argument (normal, depth or alpha)");
    if (!t) return rt::refuse(call, "t is NULL");
    if (int rc = rt::image_size_refused(call, width, height)) return rc;
    const int given = (prev_linear_rgb != nullptr) + (prev_moment2_rgb != nullptr) + (prev_length != nullptr) + (prev_normal != nullptr) +
                      (prev_depth != nullptr) + (prev_alpha != nullptr);
    const bool has_history = given == 6;
    if (given != 0 && given != 6) {
        return rt::refuse(call, "the prev_* arrays go together: prev_linear_rgb, prev_moment2_rgb, prev_length, prev_normal, prev_depth and prev_alpha all, or none");
    }
    if (has_history && !prev_cam) return rt::refuse(call, "prev_cam is NULL beside a history");
    if (int rc = rt::temporal_refuse_params(call, "t->", *t)) return rc;
    if (!v) return rt::refuse(call, "v is NULL");
    if (int rc = rt::variance_refuse_params(call, "v->", *v)) return rc;
    const rt::TemporalParams prm = rt::history_temporal_params(cam, has_history ? prev_cam : nullptr, *t, false);
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
    const char* const call = "temporal_clamp";
    if (!cam) return rt::refuse(call, "cam is NULL");
    if (!linear_rgb) return rt::refuse(call, "linear_rgb is NULL");
    if (!normal || !depth || !alpha) return rt::refuse(call, "NULL argument (normal, depth or alpha)");
    if (!t) return rt::refuse(call, "t is NULL");
    if (int rc = rt::image_size_refused(call, width, height)) return rc;
    const int given = (prev_linear_rgb != nullptr) + (prev_moment2_rgb != nullptr) + (prev_length != nullptr) + (prev_normal != nullptr) +
                      (prev_depth != nullptr) + (prev_alpha != nullptr);
    const bool has_history = given == 6;
    if (given != 0 && given != 6) {
        return rt::refuse(call, "the prev_* arrays go together: prev_linear_rgb, prev_moment2_rgb, prev_length, prev_normal, prev_depth and prev_alpha all, or none");
    }
    if (has_history && !prev_cam) return rt::refuse(call, "prev_cam is NULL beside a history");
    if (int rc = rt::temporal_refuse_params(call, "t->", *t)) return rc;
    if (!v) return rt::refuse(call, "v is NULL");
    if (int rc = rt::variance_refuse_params(call, "v->", *v)) return rc;
    if (int rc = rt::clamp_refuse_params(call, k)) return rc;
    const rt::TemporalParams prm = rt::history_temporal_params(cam, has_history ? prev_cam : nullptr, *t, false);
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
    const char* const call = "temporal_probe";
    if (!cam) return rt::refuse(call, "cam is NULL");
    if (!normal || !depth || !alpha) return rt::refuse(call, "NULL argument (normal, depth or alpha)");
    if (!t) return rt::refuse(call, "t is NULL");
    if (int rc = rt::image_size_refused(call, width, height)) return rc;
    const int given = (prev_length != nullptr) + (prev_normal != nullptr) + (prev_depth != nullptr) + (prev_alpha != nullptr);
    const bool has_history = given == 4;
    if (given != 0 && given != 4) return rt::refuse(call, "the prev_* arrays go together: prev_length, prev_normal, prev_depth and prev_alpha all, or none");
    if (has_history && !prev_cam) return rt::refuse(call, "prev_cam is NULL beside a history");
    if (int rc = rt::temporal_refuse_params(call, "t->", *t)) return rc;
    if (int rc = rt::sampling_refuse_params(call, a)) return rc;
    const rt::TemporalParams prm = rt::history_temporal_params(cam, has_history ? prev_cam : nullptr, *t, false);
    return rt::probe_device(width, height, prm, rt::sampling_params(a->boost, a->fill), normal, depth, alpha, prev_length, prev_normal, prev_depth, prev_alpha,
                            out_length, out_prev_xy, out_multiplier, kernel_ms);
}

int rttnw_reconstruct(uint32_t width, uint32_t height, const double* linear_rgb, const double* variance_rgb, const uint8_t* valid, const double* albedo,
                      const double* normal, const double* depth, const double* alpha, const rttnw_denoise_params* d, double* out_linear_rgb,
                      uint8_t* out_rgba8, double* out_variance_rgb, uint8_t* out_valid, double* kernel_ms) {
    // rttnw_denoise's refusals, with its codes, and the flags'
    const char* const call = "reconstruct";
    if (!linear_rgb || !albedo || !normal || !depth || !alpha || !d) return rt::refuse(call, "NULL argument (linear_rgb, albedo, normal, depth, alpha or d)");
    if (!valid) return rt::refuse(call, "valid is NULL");
    if (int rc = rt::image_size_refused(call, width, height)) return rc;
    if (int rc = rt::denoise_refuse_params(call, "d->", *d)) return rc;
    const rt::DenoiseParams prm = rt::denoise_params(d->sigma_luminance, d->sigma_normal, d->sigma_depth, variance_rgb != nullptr);
    return rt::atrous_device(call, width, height, linear_rgb, variance_rgb, valid, albedo, normal, depth, alpha, d->iterations, prm, out_linear_rgb,
                             out_rgba8, out_variance_rgb, out_valid, kernel_ms);
}

} // extern "C"
