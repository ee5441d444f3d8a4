//! `include/rttnw_hip.h` in Rust: every struct `#[repr(C)]` with the header's field order, every entry point.
//! Reference items each call replaces are cited in the header (file:line of luliic2/rttnw).
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_int, c_void};

pub const RTTNW_ABI_VERSION: c_int = 3;

/// Opaque scene handle.
#[repr(C)]
pub struct rttnw_scene {
    _private: [u8; 0],
}
pub type rttnw_id = i32;

// enum rttnw_status
pub const RTTNW_OK: c_int = 0;
pub const RTTNW_ERR_INVALID: c_int = -1;
pub const RTTNW_ERR_STATE: c_int = -2;
pub const RTTNW_ERR_UNSUPPORTED: c_int = -3;
pub const RTTNW_ERR_HIP: c_int = -4;
pub const RTTNW_ERR_NOMEM: c_int = -5;
// enum rttnw_plane
pub const RTTNW_XY: c_int = 0;
pub const RTTNW_XZ: c_int = 1;
pub const RTTNW_YZ: c_int = 2;
// enum rttnw_precision
pub const RTTNW_F64: u32 = 0;
pub const RTTNW_F32: u32 = 1;
pub const RTTNW_F64_STRICT: u32 = 2;
pub const RTTNW_QUIRK_YROTATE_BACKROT: u32 = 1;
pub const RTTNW_QUIRKS_REFERENCE: u32 = RTTNW_QUIRK_YROTATE_BACKROT;
pub const RTTNW_BVH_HOST_SAH: u32 = 0;
pub const RTTNW_BVH_DEVICE_LBVH: u32 = 1;
pub const RTTNW_BVH_DEVICE_SAH: u32 = 2;
pub const RTTNW_BVH_AUTO: u32 = 3;
pub const RTTNW_BVH_AUTO_DEVICE_LEAVES: u32 = 100000;
pub const RTTNW_ADAPTIVE_STATE_MAGIC: u32 = 1381256791;
pub const RTTNW_ADAPTIVE_STATE_VERSION: u32 = 1;
pub const RTTNW_ADAPTIVE_STATE_HEADER: u32 = 64;
pub const RTTNW_ADAPTIVE_STATE_RECORD: u32 = 12;

/// `CameraDescriptor` — src/math/camera.rs:5-15
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct rttnw_camera_desc {
    pub lookfrom: [f64; 3],
    pub lookat: [f64; 3],
    pub view_up: [f64; 3],
    pub vertical_fov: f64,
    pub aspect_ratio: f64,
    pub aperture: f64,
    pub focus_distance: f64,
    pub open_time: f64,
    pub close_time: f64,
}

/// What `render()` hard-codes or takes as arguments — src/main.rs:58,184-197,216,33
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct rttnw_params {
    pub width: u32,
    pub height: u32,
    pub spp: u32,
    pub max_depth: u32,
    pub t_min: f64,
    pub background: [f64; 3],
    pub seed: u64,
    pub precision: u32,
    pub quirks: u32,
    pub spp_chunk: u32,
    pub tile_rank: u32,
    pub tile_world: u32,
    pub collect_counters: u32,
    pub sample_begin: u32,
    pub reserved0: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct rttnw_stats {
    pub samples: u64,
    pub rays: u64,
    pub nodes_visited: u64,
    pub prims_tested: u64,
    pub texel_fetches: u64,
    pub kernel_ms: f64,
    pub n_nodes: u32,
    pub n_prims: u32,
    pub scene_bytes: u32,
    pub reserved: u32,
}

/// The stopping rule of `rttnw_render_adaptive` (include/rttnw_hip.h states the contract).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct rttnw_adaptive {
    pub pass_spp: u32,
    pub reserved0: u32,
    pub rel_error: f64,
    pub abs_error: f64,
}

/// The parameters of `rttnw_denoise` (include/rttnw_hip.h states the contract); a sigma of 0 is the library default.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct rttnw_denoise_params {
    pub iterations: u32,
    pub reserved0: u32,
    pub sigma_luminance: f64,
    pub sigma_normal: f64,
    pub sigma_depth: f64,
}

/// The parameters of `rttnw_denoise_nlm` (include/rttnw_hip.h states the contract); 0 is the library default.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct rttnw_nlm_params {
    pub search_radius: u32,
    pub patch_radius: u32,
    pub k: f64,
    pub reserved0: u32,
    pub reserved1: u32,
}

/// The parameters of `rttnw_denoise_regress` (include/rttnw_hip.h states the contract); a radius, `k` or `ridge` of 0 is the library default;
/// `features` holds the bits 1 (albedo), 2 (normal), 4 (depth) and has no default: 0 means no regressor.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct rttnw_regress_params {
    pub search_radius: u32,
    pub patch_radius: u32,
    pub k: f64,
    pub ridge: f64,
    pub features: u32,
    pub demodulate: u32,
    pub reserved0: u32,
    pub reserved1: u32,
}

/// The parameters of `rttnw_denoise_select` (include/rttnw_hip.h states the contract); a radius of 0 is the library default, and
/// `use_default_margin != 0` takes the default margin (0.01) and ignores `margin`: a margin of 0 is a margin of 0.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct rttnw_select_params {
    pub error_radius: u32,
    pub blend_radius: u32,
    pub margin: f64,
    pub use_default_margin: u32,
    pub reserved0: u32,
}

/// The parameters of `rttnw_temporal_accumulate` (include/rttnw_hip.h states the contract); a 0 is the library default (32 frames, a relative
/// depth tolerance of 0.05, a normalised normal product of 0.9), and `normal_min` -1 switches the normal test off.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct rttnw_temporal_params {
    pub max_history: u32,
    pub reserved0: u32,
    pub depth_tolerance: f64,
    pub normal_min: f64,
}

/// What `rttnw_temporal_variance` takes beside `rttnw_temporal_params` (include/rttnw_hip.h states the contract); a 0 is the library default (a
/// history of 4 frames is trusted, a window of radius 3, `rttnw_denoise`'s sigmas for normal and depth).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct rttnw_variance_params {
    pub min_temporal: u32,
    pub radius: u32,
    pub sigma_normal: f64,
    pub sigma_depth: f64,
    pub reserved0: u32,
    pub reserved1: u32,
}

/// What `rttnw_temporal_clamp` takes beside the two blocks of `rttnw_temporal_variance`, and `rttnw_svgf_set_clamp` alone (include/rttnw_hip.h states
/// the contract); a 0 is the library default (a window of radius 3, one standard deviation, `rttnw_denoise`'s sigmas); a `gamma` of +inf never clips.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct rttnw_clamp_params {
    pub radius: u32,
    pub reserved0: u32,
    pub gamma: f64,
    pub sigma_normal: f64,
    pub sigma_depth: f64,
}

/// What `rttnw_temporal_probe` takes beside `rttnw_temporal_params`, and `rttnw_svgf_set_sampling` alone (include/rttnw_hip.h states the contract);
/// a 0 is the library default (a boost of 8, a fill of 8.0).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct rttnw_sampling_params {
    pub boost: u32,
    pub reserved0: u32,
    pub fill: f64,
}

/// Opaque handle of the SVGF loop (`rttnw_svgf_create`): a sequence's history on the device.
#[repr(C)]
pub struct rttnw_svgf {
    _private: [u8; 0],
}

/// The settings of an `rttnw_svgf` handle (include/rttnw_hip.h states the contract): the loop's own, then the three stages' parameter blocks, in
/// which a 0 is that stage's default.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct rttnw_svgf_params {
    pub feedback_iterations: u32,
    pub demodulate: u32,
    pub feature_spp: u32,
    pub reserved0: u32,
    pub t: rttnw_temporal_params,
    pub v: rttnw_variance_params,
    pub d: rttnw_denoise_params,
}

/// The host arrays a call of `rttnw_svgf_push` / `rttnw_svgf_frame` fills; a null pointer is an output not asked for.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct rttnw_svgf_out {
    pub linear_rgb: *mut f64,
    pub rgba8: *mut u8,
    pub accumulated_rgb: *mut f64,
    pub variance_rgb: *mut f64,
    pub filtered_variance_rgb: *mut f64,
    pub length: *mut f64,
    pub prev_xy: *mut f64,
    pub moment1_rgb: *mut f64,
    pub moment2_rgb: *mut f64,
    pub history_rgb: *mut f64,
    pub raw_rgb: *mut f64,
    pub albedo: *mut f64,
    pub normal: *mut f64,
    pub depth: *mut f64,
    pub alpha: *mut f64,
    pub image_ms: *mut f64,
}

/// What `rttnw_render_adaptive_denoised` takes beside the stopping rule (include/rttnw_hip.h states the contract).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct rttnw_guided {
    pub feature_spp: u32,
    pub reserved0: u32,
    pub denoise: rttnw_denoise_params,
}

/// What `rttnw_render_preview` takes beside the stopping rule (include/rttnw_hip.h states the contract).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct rttnw_preview {
    pub level: u32,
    pub feature_spp: u32,
    pub denoise: rttnw_denoise_params,
}

/// What `rttnw_render_adaptive_budget` takes beside the stopping rule (include/rttnw_hip.h states the contract).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct rttnw_budget {
    pub samples: u64,
    pub round_pixels: u32,
    pub reserved0: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct rttnw_tile_layout {
    pub tiles_x: u32,
    pub tiles_y: u32,
    pub n_tiles: u32,
    pub tiles_per_rank: u32,
    pub pixels_per_rank: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct rttnw_build_info {
    pub builder: u32,
    pub n_nodes: u32,
    pub n_prims: u32,
    pub stack_depth: u32,
    pub lower_ms: f64,
    pub device_ms: f64,
}

/// Scene-building entry points as a table (`rttnw_builder()`), in the header's order.
#[repr(C)]
pub struct rttnw_builder_api {
    pub scene_create: Option<unsafe extern "C" fn(u64, *mut *mut rttnw_scene) -> c_int>,
    pub scene_destroy: Option<unsafe extern "C" fn(*mut rttnw_scene)>,
    pub tex_solid: Option<unsafe extern "C" fn(*mut rttnw_scene, f64, f64, f64) -> rttnw_id>,
    pub tex_checker: Option<unsafe extern "C" fn(*mut rttnw_scene, rttnw_id, rttnw_id) -> rttnw_id>,
    pub tex_noise: Option<unsafe extern "C" fn(*mut rttnw_scene, f64) -> rttnw_id>,
    pub tex_image_rgba8: Option<unsafe extern "C" fn(*mut rttnw_scene, *const u8, u32, u32) -> rttnw_id>,
    pub mat_lambertian: Option<unsafe extern "C" fn(*mut rttnw_scene, rttnw_id) -> rttnw_id>,
    pub mat_metal: Option<unsafe extern "C" fn(*mut rttnw_scene, f64, f64, f64, f64) -> rttnw_id>,
    pub mat_dielectric: Option<unsafe extern "C" fn(*mut rttnw_scene, f64) -> rttnw_id>,
    pub mat_diffuse_light: Option<unsafe extern "C" fn(*mut rttnw_scene, rttnw_id) -> rttnw_id>,
    pub mat_isotropic: Option<unsafe extern "C" fn(*mut rttnw_scene, rttnw_id) -> rttnw_id>,
    pub sphere: Option<unsafe extern "C" fn(*mut rttnw_scene, *const f64, f64, rttnw_id) -> rttnw_id>,
    pub moving_sphere: Option<unsafe extern "C" fn(*mut rttnw_scene, *const f64, *const f64, f64, f64, f64, rttnw_id) -> rttnw_id>,
    pub rectangle: Option<unsafe extern "C" fn(*mut rttnw_scene, c_int, f64, f64, f64, f64, f64, rttnw_id) -> rttnw_id>,
    pub cube: Option<unsafe extern "C" fn(*mut rttnw_scene, *const f64, *const f64, rttnw_id) -> rttnw_id>,
    pub list: Option<unsafe extern "C" fn(*mut rttnw_scene) -> rttnw_id>,
    pub list_push: Option<unsafe extern "C" fn(*mut rttnw_scene, rttnw_id, rttnw_id) -> c_int>,
    pub bvh_tree: Option<unsafe extern "C" fn(*mut rttnw_scene, rttnw_id) -> rttnw_id>,
    pub translate: Option<unsafe extern "C" fn(*mut rttnw_scene, rttnw_id, *const f64) -> rttnw_id>,
    pub rotate_y: Option<unsafe extern "C" fn(*mut rttnw_scene, rttnw_id, f64) -> rttnw_id>,
    pub constant_medium: Option<unsafe extern "C" fn(*mut rttnw_scene, rttnw_id, f64, rttnw_id) -> rttnw_id>,
    pub scene_set_world: Option<unsafe extern "C" fn(*mut rttnw_scene, rttnw_id) -> c_int>,
    pub scene_commit: Option<unsafe extern "C" fn(*mut rttnw_scene) -> c_int>,
    pub last_error: Option<unsafe extern "C" fn() -> *const c_char>,
}

extern "C" {
    // ---- lifecycle
    pub fn rttnw_scene_create(scene_seed: u64, out: *mut *mut rttnw_scene) -> c_int;
    pub fn rttnw_scene_destroy(scene: *mut rttnw_scene);
    // ---- textures (texture.rs)
    pub fn rttnw_tex_solid(s: *mut rttnw_scene, r: f64, g: f64, b: f64) -> rttnw_id;
    pub fn rttnw_tex_checker(s: *mut rttnw_scene, odd: rttnw_id, even: rttnw_id) -> rttnw_id;
    pub fn rttnw_tex_noise(s: *mut rttnw_scene, scale: f64) -> rttnw_id;
    pub fn rttnw_tex_image_rgba8(s: *mut rttnw_scene, rgba: *const u8, w: u32, h: u32) -> rttnw_id;
    // ---- materials (material.rs)
    pub fn rttnw_mat_lambertian(s: *mut rttnw_scene, tex: rttnw_id) -> rttnw_id;
    pub fn rttnw_mat_metal(s: *mut rttnw_scene, r: f64, g: f64, b: f64, fuzz: f64) -> rttnw_id;
    pub fn rttnw_mat_dielectric(s: *mut rttnw_scene, refraction_index: f64) -> rttnw_id;
    pub fn rttnw_mat_diffuse_light(s: *mut rttnw_scene, tex: rttnw_id) -> rttnw_id;
    pub fn rttnw_mat_isotropic(s: *mut rttnw_scene, tex: rttnw_id) -> rttnw_id;
    // ---- hittables (hittable.rs)
    pub fn rttnw_sphere(s: *mut rttnw_scene, center: *const f64, radius: f64, mat: rttnw_id) -> rttnw_id;
    pub fn rttnw_moving_sphere(s: *mut rttnw_scene, center0: *const f64, center1: *const f64, time0: f64, time1: f64, radius: f64, mat: rttnw_id) -> rttnw_id;
    pub fn rttnw_rectangle(s: *mut rttnw_scene, plane: c_int, a0: f64, a1: f64, b0: f64, b1: f64, k: f64, mat: rttnw_id) -> rttnw_id;
    pub fn rttnw_cube(s: *mut rttnw_scene, box_min: *const f64, box_max: *const f64, mat: rttnw_id) -> rttnw_id;
    pub fn rttnw_list(s: *mut rttnw_scene) -> rttnw_id;
    pub fn rttnw_list_push(s: *mut rttnw_scene, list: rttnw_id, item: rttnw_id) -> c_int;
    pub fn rttnw_bvh_tree(s: *mut rttnw_scene, list: rttnw_id) -> rttnw_id;
    pub fn rttnw_translate(s: *mut rttnw_scene, item: rttnw_id, offset: *const f64) -> rttnw_id;
    pub fn rttnw_rotate_y(s: *mut rttnw_scene, item: rttnw_id, angle_degrees: f64) -> rttnw_id;
    pub fn rttnw_constant_medium(s: *mut rttnw_scene, boundary: rttnw_id, density: f64, tex: rttnw_id) -> rttnw_id;
    pub fn rttnw_hittable_bounds(s: *const rttnw_scene, hittable: rttnw_id, initial_time: f64, final_time: f64, out_min_max: *mut f64) -> c_int;
    pub fn rttnw_scene_set_world(s: *mut rttnw_scene, world_list: rttnw_id) -> c_int;
    pub fn rttnw_scene_set_bvh_builder(s: *mut rttnw_scene, builder: u32) -> c_int;
    pub fn rttnw_scene_commit(s: *mut rttnw_scene) -> c_int;
    // ---- render (main.rs, camera.rs)
    pub fn rttnw_tile_layout_get(width: u32, height: u32, world: u32, out: *mut rttnw_tile_layout) -> c_int;
    pub fn rttnw_render(s: *mut rttnw_scene, cam: *const rttnw_camera_desc, p: *const rttnw_params, out_linear_rgb: *mut f64, out_rgba8: *mut u8, stats: *mut rttnw_stats) -> c_int;
    pub fn rttnw_render_multi(s: *mut rttnw_scene, cam: *const rttnw_camera_desc, p: *const rttnw_params, ngpu: u32, device_ids: *const i32, out_linear_rgb: *mut f64, out_rgba8: *mut u8, stats: *mut rttnw_stats) -> c_int;
    pub fn rttnw_render_adaptive(s: *mut rttnw_scene, cam: *const rttnw_camera_desc, p: *const rttnw_params, a: *const rttnw_adaptive, out_linear_rgb: *mut f64, out_rgba8: *mut u8, out_spp: *mut u32, out_stderr_rgb: *mut f64, stats: *mut rttnw_stats) -> c_int;
    pub fn rttnw_render_adaptive_multi(s: *mut rttnw_scene, cam: *const rttnw_camera_desc, p: *const rttnw_params, a: *const rttnw_adaptive, ngpu: u32, device_ids: *const i32, out_linear_rgb: *mut f64, out_rgba8: *mut u8, out_spp: *mut u32, out_stderr_rgb: *mut f64, stats: *mut rttnw_stats) -> c_int;
    pub fn rttnw_adaptive_state_doubles(width: u32, height: u32) -> u64;
    pub fn rttnw_render_adaptive_resume(s: *mut rttnw_scene, cam: *const rttnw_camera_desc, p: *const rttnw_params, a: *const rttnw_adaptive, ngpu: u32, device_ids: *const i32, state_in: *const f64, state_out: *mut f64, out_linear_rgb: *mut f64, out_rgba8: *mut u8, out_spp: *mut u32, out_stderr_rgb: *mut f64, stats: *mut rttnw_stats) -> c_int;
    pub fn rttnw_render_adaptive_region(s: *mut rttnw_scene, cam: *const rttnw_camera_desc, p: *const rttnw_params, a: *const rttnw_adaptive, x0: u32, y0: u32, x1: u32, y1: u32, mask: *const u8, ngpu: u32, device_ids: *const i32, state_in: *const f64, state_out: *mut f64, out_linear_rgb: *mut f64, out_rgba8: *mut u8, out_spp: *mut u32, out_stderr_rgb: *mut f64, stats: *mut rttnw_stats) -> c_int;
    pub fn rttnw_render_adaptive_denoised(s: *mut rttnw_scene, cam: *const rttnw_camera_desc, p: *const rttnw_params, a: *const rttnw_adaptive, g: *const rttnw_guided, out_linear_rgb: *mut f64, out_rgba8: *mut u8, out_spp: *mut u32, out_stderr_rgb: *mut f64, out_raw_linear_rgb: *mut f64, out_raw_stderr_rgb: *mut f64, state_out: *mut f64, stats: *mut rttnw_stats) -> c_int;
    pub fn rttnw_render_features(s: *mut rttnw_scene, cam: *const rttnw_camera_desc, p: *const rttnw_params, out_albedo: *mut f64, out_normal: *mut f64, out_depth: *mut f64, out_alpha: *mut f64, stats: *mut rttnw_stats) -> c_int;
    pub fn rttnw_render_region(s: *mut rttnw_scene, cam: *const rttnw_camera_desc, p: *const rttnw_params, x0: u32, y0: u32, x1: u32, y1: u32, mask: *const u8, out_linear_rgb: *mut f64, out_rgba8: *mut u8, stats: *mut rttnw_stats) -> c_int;
    pub fn rttnw_denoise(width: u32, height: u32, linear_rgb: *const f64, variance_rgb: *const f64, albedo: *const f64, normal: *const f64, depth: *const f64, alpha: *const f64, d: *const rttnw_denoise_params, out_linear_rgb: *mut f64, out_rgba8: *mut u8, out_variance_rgb: *mut f64, kernel_ms: *mut f64) -> c_int;
    pub fn rttnw_denoise_nlm(width: u32, height: u32, half_a: *const f64, half_b: *const f64, var_a: *const f64, var_b: *const f64, d: *const rttnw_nlm_params, out_linear_rgb: *mut f64, out_rgba8: *mut u8, out_half_a: *mut f64, out_half_b: *mut f64, out_error_rgb: *mut f64, kernel_ms: *mut f64) -> c_int;
    pub fn rttnw_denoise_select(width: u32, height: u32, half_a: *const f64, half_b: *const f64, var_a: *const f64, var_b: *const f64, albedo: *const f64, normal: *const f64, depth: *const f64, alpha: *const f64, dn: *const rttnw_denoise_params, nl: *const rttnw_nlm_params, sel: *const rttnw_select_params, out_linear_rgb: *mut f64, out_rgba8: *mut u8, out_blend: *mut f64, out_feature_rgb: *mut f64, out_nlm_rgb: *mut f64, out_error_rgb: *mut f64, kernel_ms: *mut f64) -> c_int;
    pub fn rttnw_denoise_regress(width: u32, height: u32, half_a: *const f64, half_b: *const f64, var_a: *const f64, var_b: *const f64, albedo: *const f64, normal: *const f64, depth: *const f64, alpha: *const f64, g: *const rttnw_regress_params, out_linear_rgb: *mut f64, out_rgba8: *mut u8, out_half_a: *mut f64, out_half_b: *mut f64, out_error_rgb: *mut f64, out_fit: *mut f64, kernel_ms: *mut f64) -> c_int;
    pub fn rttnw_temporal_accumulate(width: u32, height: u32, cam: *const rttnw_camera_desc, prev_cam: *const rttnw_camera_desc, linear_rgb: *const f64, variance_rgb: *const f64, normal: *const f64, depth: *const f64, alpha: *const f64, prev_linear_rgb: *const f64, prev_variance_rgb: *const f64, prev_length: *const f64, prev_normal: *const f64, prev_depth: *const f64, prev_alpha: *const f64, t: *const rttnw_temporal_params, out_linear_rgb: *mut f64, out_rgba8: *mut u8, out_variance_rgb: *mut f64, out_length: *mut f64, out_prev_xy: *mut f64, kernel_ms: *mut f64) -> c_int;
    pub fn rttnw_temporal_clamp(width: u32, height: u32, cam: *const rttnw_camera_desc, prev_cam: *const rttnw_camera_desc, linear_rgb: *const f64, normal: *const f64, depth: *const f64, alpha: *const f64, prev_linear_rgb: *const f64, prev_moment2_rgb: *const f64, prev_length: *const f64, prev_normal: *const f64, prev_depth: *const f64, prev_alpha: *const f64, t: *const rttnw_temporal_params, v: *const rttnw_variance_params, k: *const rttnw_clamp_params, out_linear_rgb: *mut f64, out_rgba8: *mut u8, out_moment2_rgb: *mut f64, out_length: *mut f64, out_prev_xy: *mut f64, out_variance_rgb: *mut f64, out_mean_rgb: *mut f64, out_sd_rgb: *mut f64, out_clipped: *mut u8, kernel_ms: *mut f64) -> c_int;
    pub fn rttnw_svgf_set_clamp(q: *mut rttnw_svgf, k: *const rttnw_clamp_params) -> c_int;
    pub fn rttnw_svgf_clipped(q: *mut rttnw_svgf, out_clipped: *mut u8) -> c_int;
    pub fn rttnw_temporal_probe(width: u32, height: u32, cam: *const rttnw_camera_desc, prev_cam: *const rttnw_camera_desc, normal: *const f64, depth: *const f64, alpha: *const f64, prev_length: *const f64, prev_normal: *const f64, prev_depth: *const f64, prev_alpha: *const f64, t: *const rttnw_temporal_params, a: *const rttnw_sampling_params, out_length: *mut f64, out_prev_xy: *mut f64, out_multiplier: *mut u8, kernel_ms: *mut f64) -> c_int;
    pub fn rttnw_svgf_set_sampling(q: *mut rttnw_svgf, a: *const rttnw_sampling_params) -> c_int;
    pub fn rttnw_svgf_samples(q: *mut rttnw_svgf, out_spp: *mut u32, out_length: *mut f64) -> c_int;
    pub fn rttnw_svgf_set_regress(q: *mut rttnw_svgf, g: *const rttnw_regress_params, variance_source: u32) -> c_int;
    pub fn rttnw_svgf_push_halves(q: *mut rttnw_svgf, cam: *const rttnw_camera_desc, half_a: *const f64, half_b: *const f64, albedo: *const f64, normal: *const f64, depth: *const f64, alpha: *const f64, out: *const rttnw_svgf_out) -> c_int;
    pub fn rttnw_svgf_halves(q: *mut rttnw_svgf, out_acc_a: *mut f64, out_acc_b: *mut f64, out_filtered_a: *mut f64, out_filtered_b: *mut f64, out_fit: *mut f64) -> c_int;
    pub fn rttnw_svgf_create(width: u32, height: u32, q: *const rttnw_svgf_params, out: *mut *mut rttnw_svgf) -> c_int;
    pub fn rttnw_svgf_destroy(q: *mut rttnw_svgf);
    pub fn rttnw_svgf_reset(q: *mut rttnw_svgf) -> c_int;
    pub fn rttnw_svgf_push(q: *mut rttnw_svgf, cam: *const rttnw_camera_desc, linear_rgb: *const f64, albedo: *const f64, normal: *const f64, depth: *const f64, alpha: *const f64, out: *const rttnw_svgf_out) -> c_int;
    pub fn rttnw_svgf_frame(q: *mut rttnw_svgf, s: *mut rttnw_scene, cam: *const rttnw_camera_desc, p: *const rttnw_params, out: *const rttnw_svgf_out, stats: *mut rttnw_stats) -> c_int;
    pub fn rttnw_temporal_variance(width: u32, height: u32, cam: *const rttnw_camera_desc, prev_cam: *const rttnw_camera_desc, linear_rgb: *const f64, normal: *const f64, depth: *const f64, alpha: *const f64, prev_linear_rgb: *const f64, prev_moment2_rgb: *const f64, prev_length: *const f64, prev_normal: *const f64, prev_depth: *const f64, prev_alpha: *const f64, t: *const rttnw_temporal_params, v: *const rttnw_variance_params, out_linear_rgb: *mut f64, out_rgba8: *mut u8, out_moment2_rgb: *mut f64, out_length: *mut f64, out_prev_xy: *mut f64, out_variance_rgb: *mut f64, kernel_ms: *mut f64) -> c_int;
    pub fn rttnw_reconstruct(width: u32, height: u32, linear_rgb: *const f64, variance_rgb: *const f64, valid: *const u8, albedo: *const f64, normal: *const f64, depth: *const f64, alpha: *const f64, d: *const rttnw_denoise_params, out_linear_rgb: *mut f64, out_rgba8: *mut u8, out_variance_rgb: *mut f64, out_valid: *mut u8, kernel_ms: *mut f64) -> c_int;
    pub fn rttnw_render_preview(s: *mut rttnw_scene, cam: *const rttnw_camera_desc, p: *const rttnw_params, a: *const rttnw_adaptive, v: *const rttnw_preview, out_linear_rgb: *mut f64, out_rgba8: *mut u8, out_valid: *mut u8, out_spp: *mut u32, out_raw_linear_rgb: *mut f64, out_raw_stderr_rgb: *mut f64, state_out: *mut f64, stats: *mut rttnw_stats) -> c_int;
    pub fn rttnw_budget_select(width: u32, height: u32, linear_rgb: *const f64, stderr_rgb: *const f64, spp: *const u32, cap: u32, rel_error: f64, abs_error: f64, max_pixels: u64, out_mask: *mut u8, out_priority: *mut f64, out_selected: *mut u64, kernel_ms: *mut f64) -> c_int;
    pub fn rttnw_render_adaptive_budget(s: *mut rttnw_scene, cam: *const rttnw_camera_desc, p: *const rttnw_params, a: *const rttnw_adaptive, b: *const rttnw_budget, state_in: *const f64, state_out: *mut f64, out_linear_rgb: *mut f64, out_rgba8: *mut u8, out_spp: *mut u32, out_stderr_rgb: *mut f64, stats: *mut rttnw_stats) -> c_int;
    pub fn rttnw_render_adaptive_budget_denoised(s: *mut rttnw_scene, cam: *const rttnw_camera_desc, p: *const rttnw_params, a: *const rttnw_adaptive, b: *const rttnw_budget, g: *const rttnw_guided, state_in: *const f64, state_out: *mut f64, out_linear_rgb: *mut f64, out_rgba8: *mut u8, out_valid: *mut u8, out_spp: *mut u32, out_stderr_rgb: *mut f64, out_raw_linear_rgb: *mut f64, out_raw_stderr_rgb: *mut f64, stats: *mut rttnw_stats) -> c_int;
    pub fn rttnw_render_tiles_device(s: *mut rttnw_scene, cam: *const rttnw_camera_desc, p: *const rttnw_params, d_packed: *mut c_void, hip_stream: *mut c_void, stats: *mut rttnw_stats) -> c_int;
    pub fn rttnw_untile_device(width: u32, height: u32, world: u32, precision: u32, d_gathered: *const c_void, d_linear_rgb: *mut c_void, d_rgba8: *mut u8, hip_stream: *mut c_void) -> c_int;
    // ---- introspection
    pub fn rttnw_abi_version() -> c_int;
    pub fn rttnw_shutdown();
    pub fn rttnw_device_count() -> c_int;
    pub fn rttnw_last_error() -> *const c_char;
    pub fn rttnw_scene_info(s: *mut rttnw_scene, out: *mut rttnw_stats) -> c_int;
    pub fn rttnw_scene_build_info(s: *const rttnw_scene, out: *mut rttnw_build_info) -> c_int;
    pub fn rttnw_debug_scene_nodes(s: *const rttnw_scene, out_nodes: *mut c_void, max_nodes: u32, top_root: *mut i32) -> c_int;
    pub fn rttnw_debug_scene_nodes4(s: *const rttnw_scene, out_nodes: *mut c_void, max_nodes: u32, top_root: *mut i32) -> c_int;
    pub fn rttnw_debug_probe_path(s: *mut rttnw_scene, cam: *const rttnw_camera_desc, p: *const rttnw_params, px: u32, row: u32, sample: u32, out: *mut f64, max_out: u32) -> c_int;
    pub fn rttnw_builder() -> *const rttnw_builder_api;
}
