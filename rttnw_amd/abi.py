"""ctypes declarations of the C ABI in include/rttnw_hip.h and include/rttnw_scenes.h.

Pure declarations: structures, status codes and the signature table used to bind a shared
library that implements the boundary.  No library is loaded here.
"""
import ctypes as C

RTTNW_OK = 0
ERR_NAMES = {-1: "RTTNW_ERR_INVALID", -2: "RTTNW_ERR_STATE", -3: "RTTNW_ERR_UNSUPPORTED",
             -4: "RTTNW_ERR_HIP", -5: "RTTNW_ERR_NOMEM"}

XY, XZ, YZ = 0, 1, 2
F64, F32, F64_STRICT = 0, 1, 2
BVH_HOST_SAH, BVH_DEVICE_LBVH, BVH_DEVICE_SAH, BVH_AUTO = 0, 1, 2, 3
ABI_VERSION = 3  # include/rttnw_hip.h RTTNW_ABI_VERSION
QUIRK_YROTATE_BACKROT = 1
QUIRKS_REFERENCE = QUIRK_YROTATE_BACKROT

c_id = C.c_int32
c_double3 = C.c_double * 3
scene_p = C.c_void_p


class CameraDesc(C.Structure):
    """`CameraDescriptor` — reference src/math/camera.rs:5-15."""
    _fields_ = [("lookfrom", c_double3), ("lookat", c_double3), ("view_up", c_double3),
                ("vertical_fov", C.c_double), ("aspect_ratio", C.c_double), ("aperture", C.c_double),
                ("focus_distance", C.c_double), ("open_time", C.c_double), ("close_time", C.c_double)]


class Params(C.Structure):
    """What `render()` hard-codes or takes as arguments — reference src/main.rs:58,184-197,216,33."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("spp", C.c_uint32), ("max_depth", C.c_uint32),
                ("t_min", C.c_double), ("background", c_double3), ("seed", C.c_uint64),
                ("precision", C.c_uint32), ("quirks", C.c_uint32), ("spp_chunk", C.c_uint32),
                ("tile_rank", C.c_uint32), ("tile_world", C.c_uint32), ("collect_counters", C.c_uint32),
                ("sample_begin", C.c_uint32), ("reserved0", C.c_uint32)]


class BuildInfo(C.Structure):
    _fields_ = [("builder", C.c_uint32), ("n_nodes", C.c_uint32), ("n_prims", C.c_uint32), ("stack_depth", C.c_uint32),
                ("lower_ms", C.c_double), ("device_ms", C.c_double)]


class Stats(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("rays", C.c_uint64), ("nodes_visited", C.c_uint64),
                ("prims_tested", C.c_uint64), ("texel_fetches", C.c_uint64), ("kernel_ms", C.c_double),
                ("n_nodes", C.c_uint32), ("n_prims", C.c_uint32), ("scene_bytes", C.c_uint32),
                ("reserved", C.c_uint32)]


class Adaptive(C.Structure):
    """`rttnw_adaptive` — the stopping rule of `rttnw_render_adaptive`."""
    _fields_ = [("pass_spp", C.c_uint32), ("reserved0", C.c_uint32), ("rel_error", C.c_double), ("abs_error", C.c_double)]


class Denoise(C.Structure):
    """`rttnw_denoise_params` — the parameters of `rttnw_denoise` (a sigma of 0: the library default)."""
    _fields_ = [("iterations", C.c_uint32), ("reserved0", C.c_uint32), ("sigma_luminance", C.c_double),
                ("sigma_normal", C.c_double), ("sigma_depth", C.c_double)]


class Nlm(C.Structure):
    """`rttnw_nlm_params` — the parameters of `rttnw_denoise_nlm` (0: the library default)."""
    _fields_ = [("search_radius", C.c_uint32), ("patch_radius", C.c_uint32), ("k", C.c_double), ("reserved0", C.c_uint32),
                ("reserved1", C.c_uint32)]


class Regress(C.Structure):
    """`rttnw_regress_params` — the parameters of `rttnw_denoise_regress` (a radius, `k` or `ridge` of 0: the library default; `features`: bits 1
    albedo, 2 normal, 4 depth, where 0 means no regressor)."""
    _fields_ = [("search_radius", C.c_uint32), ("patch_radius", C.c_uint32), ("k", C.c_double), ("ridge", C.c_double), ("features", C.c_uint32),
                ("demodulate", C.c_uint32), ("reserved0", C.c_uint32), ("reserved1", C.c_uint32)]


class Select(C.Structure):
    """`rttnw_select_params` — the parameters of `rttnw_denoise_select` (a radius of 0: the library default; `use_default_margin` != 0: the
    default margin, `margin` ignored)."""
    _fields_ = [("error_radius", C.c_uint32), ("blend_radius", C.c_uint32), ("margin", C.c_double), ("use_default_margin", C.c_uint32),
                ("reserved0", C.c_uint32)]


class Temporal(C.Structure):
    """`rttnw_temporal_params` — the parameters of `rttnw_temporal_accumulate` (a 0: the library default; `normal_min` -1: no normal test)."""
    _fields_ = [("max_history", C.c_uint32), ("reserved0", C.c_uint32), ("depth_tolerance", C.c_double), ("normal_min", C.c_double)]


class Variance(C.Structure):
    """`rttnw_variance_params` — what `rttnw_temporal_variance` takes beside `rttnw_temporal_params` (a 0: the library default)."""
    _fields_ = [("min_temporal", C.c_uint32), ("radius", C.c_uint32), ("sigma_normal", C.c_double), ("sigma_depth", C.c_double),
                ("reserved0", C.c_uint32), ("reserved1", C.c_uint32)]


class Clamp(C.Structure):
    """`rttnw_clamp_params` — what `rttnw_temporal_clamp` takes beside the two blocks of `rttnw_temporal_variance`, and `rttnw_svgf_set_clamp` alone
    (a 0: the library default; a `gamma` of +inf never clips)."""
    _fields_ = [("radius", C.c_uint32), ("reserved0", C.c_uint32), ("gamma", C.c_double), ("sigma_normal", C.c_double), ("sigma_depth", C.c_double)]


class Sampling(C.Structure):
    """`rttnw_sampling_params` — what `rttnw_temporal_probe` takes beside `rttnw_temporal_params`, and `rttnw_svgf_set_sampling` alone: the largest
    multiple of the frame's spp a pixel may get and the fill the boost aims at (a 0: the library default, 8 and 8.0)."""
    _fields_ = [("boost", C.c_uint32), ("reserved0", C.c_uint32), ("fill", C.c_double)]


class Svgf(C.Structure):
    """`rttnw_svgf_params` — the settings of an `rttnw_svgf` handle: the loop's own, then the three stages' blocks (a 0: that stage's default)."""
    _fields_ = [("feedback_iterations", C.c_uint32), ("demodulate", C.c_uint32), ("feature_spp", C.c_uint32), ("reserved0", C.c_uint32),
                ("t", Temporal), ("v", Variance), ("d", Denoise)]


SVGF_OUTPUTS = ("linear_rgb", "rgba8", "accumulated_rgb", "variance_rgb", "filtered_variance_rgb", "length", "prev_xy", "moment1_rgb", "moment2_rgb",
                "history_rgb", "raw_rgb", "albedo", "normal", "depth", "alpha", "image_ms")


class SvgfOut(C.Structure):
    """`rttnw_svgf_out` — the host arrays a call of `rttnw_svgf_push` / `rttnw_svgf_frame` fills, each optional."""
    _fields_ = [(name, C.c_void_p) for name in SVGF_OUTPUTS]


class Guided(C.Structure):
    """`rttnw_guided` — what `rttnw_render_adaptive_denoised` and `rttnw_render_adaptive_budget_denoised` take beside the stopping rule: the
    features' samples and the filter."""
    _fields_ = [("feature_spp", C.c_uint32), ("reserved0", C.c_uint32), ("denoise", Denoise)]


class Preview(C.Structure):
    """`rttnw_preview` — what `rttnw_render_preview` takes beside the stopping rule: the lattice, the features' samples and the filter."""
    _fields_ = [("level", C.c_uint32), ("feature_spp", C.c_uint32), ("denoise", Denoise)]


class Budget(C.Structure):
    """`rttnw_budget` — what `rttnw_render_adaptive_budget` takes beside the stopping rule: the samples the call may trace and the size of a round."""
    _fields_ = [("samples", C.c_uint64), ("round_pixels", C.c_uint32), ("reserved0", C.c_uint32)]


class TileLayout(C.Structure):
    _fields_ = [("tiles_x", C.c_uint32), ("tiles_y", C.c_uint32), ("n_tiles", C.c_uint32),
                ("tiles_per_rank", C.c_uint32), ("pixels_per_rank", C.c_uint32)]


class SceneSetup(C.Structure):
    """Per-scene camera/size table entry — reference src/main.rs:66-183."""
    _fields_ = [("camera", CameraDesc), ("background", c_double3), ("width", C.c_uint32),
                ("height", C.c_uint32), ("spp", C.c_uint32), ("scene_number", C.c_uint32)]


_dp = C.POINTER(C.c_double)
_u8p = C.POINTER(C.c_uint8)

# (name, restype, argtypes) of the scene-building entry points, in rttnw_builder_api order.
BUILDER_FUNCS = [
    ("scene_create", C.c_int, [C.c_uint64, C.POINTER(scene_p)]),
    ("scene_destroy", None, [scene_p]),
    ("tex_solid", c_id, [scene_p, C.c_double, C.c_double, C.c_double]),
    ("tex_checker", c_id, [scene_p, c_id, c_id]),
    ("tex_noise", c_id, [scene_p, C.c_double]),
    ("tex_image_rgba8", c_id, [scene_p, C.c_void_p, C.c_uint32, C.c_uint32]),
    ("mat_lambertian", c_id, [scene_p, c_id]),
    ("mat_metal", c_id, [scene_p, C.c_double, C.c_double, C.c_double, C.c_double]),
    ("mat_dielectric", c_id, [scene_p, C.c_double]),
    ("mat_diffuse_light", c_id, [scene_p, c_id]),
    ("mat_isotropic", c_id, [scene_p, c_id]),
    ("sphere", c_id, [scene_p, c_double3, C.c_double, c_id]),
    ("moving_sphere", c_id, [scene_p, c_double3, c_double3, C.c_double, C.c_double, C.c_double, c_id]),
    ("rectangle", c_id, [scene_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, c_id]),
    ("cube", c_id, [scene_p, c_double3, c_double3, c_id]),
    ("list", c_id, [scene_p]),
    ("list_push", C.c_int, [scene_p, c_id, c_id]),
    ("bvh_tree", c_id, [scene_p, c_id]),
    ("translate", c_id, [scene_p, c_id, c_double3]),
    ("rotate_y", c_id, [scene_p, c_id, C.c_double]),
    ("constant_medium", c_id, [scene_p, c_id, C.c_double, c_id]),
    ("scene_set_world", C.c_int, [scene_p, c_id]),
    ("scene_commit", C.c_int, [scene_p]),
    ("last_error", C.c_char_p, []),
]

# render / introspection entry points of the product library (prefix rttnw_)
PRODUCT_FUNCS = [
    ("tile_layout_get", C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(TileLayout)]),
    ("render", C.c_int, [scene_p, C.POINTER(CameraDesc), C.POINTER(Params), C.c_void_p, C.c_void_p,
                         C.POINTER(Stats)]),
    ("render_multi", C.c_int, [scene_p, C.POINTER(CameraDesc), C.POINTER(Params), C.c_uint32, C.POINTER(C.c_int32), C.c_void_p,
                               C.c_void_p, C.c_void_p]),
    ("render_adaptive", C.c_int, [scene_p, C.POINTER(CameraDesc), C.POINTER(Params), C.POINTER(Adaptive), C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    ("render_adaptive_multi", C.c_int, [scene_p, C.POINTER(CameraDesc), C.POINTER(Params), C.POINTER(Adaptive), C.c_uint32, C.POINTER(C.c_int32),
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("adaptive_state_doubles", C.c_uint64, [C.c_uint32, C.c_uint32]),
    ("render_adaptive_resume", C.c_int, [scene_p, C.POINTER(CameraDesc), C.POINTER(Params), C.POINTER(Adaptive), C.c_uint32, C.POINTER(C.c_int32),
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("render_adaptive_region", C.c_int, [scene_p, C.POINTER(CameraDesc), C.POINTER(Params), C.POINTER(Adaptive), C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    ("render_adaptive_denoised", C.c_int, [scene_p, C.POINTER(CameraDesc), C.POINTER(Params), C.POINTER(Adaptive), C.POINTER(Guided), C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    ("render_features", C.c_int, [scene_p, C.POINTER(CameraDesc), C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.POINTER(Stats)]),
    ("render_region", C.c_int, [scene_p, C.POINTER(CameraDesc), C.POINTER(Params), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    ("denoise", C.c_int, [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                          C.POINTER(Denoise), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    ("reconstruct", C.c_int, [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.POINTER(Denoise), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    ("denoise_nlm", C.c_int, [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Nlm), C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    ("denoise_select", C.c_int, [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.POINTER(Denoise), C.POINTER(Nlm), C.POINTER(Select), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    ("denoise_regress", C.c_int, [C.c_uint32, C.c_uint32] + [C.c_void_p] * 8 + [C.POINTER(Regress)] + [C.c_void_p] * 6 + [C.POINTER(C.c_double)]),
    ("temporal_accumulate", C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(CameraDesc), C.POINTER(CameraDesc)] + [C.c_void_p] * 11 +
                                     [C.POINTER(Temporal)] + [C.c_void_p] * 5 + [C.POINTER(C.c_double)]),
    ("temporal_variance", C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(CameraDesc), C.POINTER(CameraDesc)] + [C.c_void_p] * 10 +
                                   [C.POINTER(Temporal), C.POINTER(Variance)] + [C.c_void_p] * 6 + [C.POINTER(C.c_double)]),
    ("svgf_create", C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(Svgf), C.POINTER(C.c_void_p)]),
    ("svgf_destroy", None, [C.c_void_p]),
    ("svgf_reset", C.c_int, [C.c_void_p]),
    ("svgf_push", C.c_int, [C.c_void_p, C.POINTER(CameraDesc)] + [C.c_void_p] * 5 + [C.POINTER(SvgfOut)]),
    ("svgf_frame", C.c_int, [C.c_void_p, scene_p, C.POINTER(CameraDesc), C.POINTER(Params), C.POINTER(SvgfOut), C.POINTER(Stats)]),
    ("temporal_clamp", C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(CameraDesc), C.POINTER(CameraDesc)] + [C.c_void_p] * 10 +
                                [C.POINTER(Temporal), C.POINTER(Variance), C.POINTER(Clamp)] + [C.c_void_p] * 9 + [C.POINTER(C.c_double)]),
    ("svgf_set_clamp", C.c_int, [C.c_void_p, C.POINTER(Clamp)]),
    ("svgf_clipped", C.c_int, [C.c_void_p, C.c_void_p]),
    ("temporal_probe", C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(CameraDesc), C.POINTER(CameraDesc)] + [C.c_void_p] * 7 +
                                [C.POINTER(Temporal), C.POINTER(Sampling)] + [C.c_void_p] * 3 + [C.POINTER(C.c_double)]),
    ("svgf_set_sampling", C.c_int, [C.c_void_p, C.POINTER(Sampling)]),
    ("svgf_samples", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("svgf_set_regress", C.c_int, [C.c_void_p, C.POINTER(Regress), C.c_uint32]),
    ("svgf_push_halves", C.c_int, [C.c_void_p, C.POINTER(CameraDesc)] + [C.c_void_p] * 6 + [C.POINTER(SvgfOut)]),
    ("svgf_halves", C.c_int, [C.c_void_p] + [C.c_void_p] * 5),
    ("render_preview", C.c_int, [scene_p, C.POINTER(CameraDesc), C.POINTER(Params), C.POINTER(Adaptive), C.POINTER(Preview), C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    ("budget_select", C.c_int, [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_double, C.c_double, C.c_uint64,
                                C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    ("render_adaptive_budget", C.c_int, [scene_p, C.POINTER(CameraDesc), C.POINTER(Params), C.POINTER(Adaptive), C.POINTER(Budget), C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    ("render_adaptive_budget_denoised", C.c_int, [scene_p, C.POINTER(CameraDesc), C.POINTER(Params), C.POINTER(Adaptive), C.POINTER(Budget),
                                                  C.POINTER(Guided), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    ("render_tiles_device", C.c_int, [scene_p, C.POINTER(CameraDesc), C.POINTER(Params), C.c_void_p,
                                      C.c_void_p, C.POINTER(Stats)]),
    ("untile_device", C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p]),
    ("abi_version", C.c_int, []),
    ("shutdown", None, []),
    ("device_count", C.c_int, []),
    ("scene_info", C.c_int, [scene_p, C.POINTER(Stats)]),
    ("scene_set_bvh_builder", C.c_int, [scene_p, C.c_uint32]),
    ("scene_build_info", C.c_int, [scene_p, C.POINTER(BuildInfo)]),
    ("hittable_bounds", C.c_int, [scene_p, c_id, C.c_double, C.c_double, _dp]),
    ("debug_scene_nodes", C.c_int, [scene_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_int32)]),
    ("debug_scene_nodes4", C.c_int, [scene_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_int32)]),
    ("builder", C.c_void_p, []),
    ("debug_probe_path", C.c_int, [scene_p, C.POINTER(CameraDesc), C.POINTER(Params), C.c_uint32, C.c_uint32,
                                   C.c_uint32, C.c_void_p, C.c_uint32]),
]

SCENES_FUNCS = [
    ("rttnw_scenes_build", C.c_int, [C.c_void_p, scene_p, C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint32,
                                     C.c_uint32, C.c_uint32, C.POINTER(SceneSetup)]),
    ("rttnw_scenes_name", C.c_char_p, [C.c_uint32]),
    ("rttnw_scenes_rng_f64", None, [C.c_uint64, C.c_uint64, C.c_uint32, _dp]),
]


class Binding:
    """Functions of one implementation of the boundary, bound by prefix (`rttnw_` = product)."""

    def __init__(self, lib, prefix, funcs):
        self.lib = lib
        self.prefix = prefix
        for name, restype, argtypes in funcs:
            fn = getattr(lib, prefix + name)
            fn.restype = restype
            fn.argtypes = argtypes
            setattr(self, name.replace("rttnw_", ""), fn)

    def add(self, funcs, prefix=None):
        for name, restype, argtypes in funcs:
            fn = getattr(self.lib, (self.prefix if prefix is None else prefix) + name)
            fn.restype = restype
            fn.argtypes = argtypes
            setattr(self, name.replace("rttnw_", ""), fn)


def exported_symbols(prefix="rttnw_"):
    """Every symbol include/rttnw_hip.h declares (used by the CPU-side export test)."""
    return [prefix + n for n, _, _ in BUILDER_FUNCS] + [prefix + n for n, _, _ in PRODUCT_FUNCS]


def vec3(x, y=None, z=None):
    if y is None:
        x, y, z = x
    return c_double3(float(x), float(y), float(z))


class RttnwError(RuntimeError):
    pass


def check(rc, binding, what=""):
    if rc is not None and rc < 0:
        msg = binding.last_error()
        raise RttnwError("%s failed: %s (%s)" % (what or "call", ERR_NAMES.get(rc, rc),
                                                 msg.decode() if msg else ""))
    return rc
