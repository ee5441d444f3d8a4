"""TEST INFRASTRUCTURE — ctypes loader for the CPU oracle (oracle/librttnw_oracle.so).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from rttnw_amd import abi
from rttnw_amd.abi import CameraDesc, Params, Stats

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "librttnw_oracle.so")
_dp = C.POINTER(C.c_double)

_PROBES = [
    ("render", C.c_int, [abi.scene_p, C.POINTER(CameraDesc), C.POINTER(Params), C.c_void_p, C.c_void_p,
                         C.POINTER(Stats), C.c_int]),
    ("render_window", C.c_int, [abi.scene_p, C.POINTER(CameraDesc), C.POINTER(Params), C.c_uint32, C.c_uint32, C.c_uint32,
                                C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats), C.c_int]),
    ("render_pixel_list", C.c_int, [abi.scene_p, C.POINTER(CameraDesc), C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_uint32,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats), C.c_int]),
    ("probe_path", C.c_int, [abi.scene_p, C.POINTER(CameraDesc), C.POINTER(Params), C.c_uint32, C.c_uint32, C.c_uint32,
                             _dp, C.c_uint32]),
    ("builder", C.c_void_p, []),
    ("scene_set_bvh_builder", C.c_int, [abi.scene_p, C.c_uint32]),
    ("probe_camera", C.c_int, [C.POINTER(CameraDesc), _dp]),
    ("probe_camera_ray", C.c_int, [C.POINTER(CameraDesc), C.c_double, C.c_double, C.c_uint64, C.c_uint64,
                                   C.c_uint64, _dp]),
    ("probe_hit", C.c_int, [abi.scene_p, abi.c_id, _dp, C.c_double, C.c_double, C.c_uint64, C.c_uint64,
                            C.c_uint64, C.c_uint32, C.c_uint32, _dp]),
    ("probe_scatter", C.c_int, [abi.scene_p, abi.c_id, _dp, _dp, C.c_uint64, C.c_uint64, C.c_uint64,
                                C.c_uint32, _dp]),
    ("probe_tex", C.c_int, [abi.scene_p, abi.c_id, C.c_double, C.c_double, _dp, _dp]),
    ("probe_perlin", C.c_int, [abi.scene_p, abi.c_id, _dp, C.c_uint32, _dp]),
    ("probe_perlin_tables", C.c_int, [abi.scene_p, abi.c_id, _dp, C.POINTER(C.c_uint32)]),
    ("probe_aabb", C.c_int, [_dp, _dp, C.c_double, C.c_double]),
    ("probe_bbox", C.c_int, [abi.scene_p, abi.c_id, C.c_double, C.c_double, _dp]),
    ("probe_schlick", C.c_double, [C.c_double, C.c_double]),
    ("probe_refract", None, [_dp, _dp, C.c_double, _dp]),
    ("probe_reflect", None, [_dp, _dp, _dp]),
    ("probe_quantise", C.c_int, [C.c_double]),
    ("probe_uniform", C.c_double, [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32]),
    ("probe_word", C.c_uint64, [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32]),
    ("probe_scene_rng", None, [C.c_uint64, C.c_uint64, C.c_uint32, _dp]),
    ("probe_sample", C.c_int, [abi.scene_p, C.POINTER(CameraDesc), C.POINTER(Params), C.c_uint32, C.c_uint32,
                               C.c_uint32, _dp]),
]

_binding = None

# rto_scene_set_bvh_builder (ORACLE-ONLY; `bvh=` of rttnw_amd.scene.build reaches it through the oracle binding): which
# topology BvhTree::hit hangs on.  The reference's builder is O(n^2 log n); MEDIAN_SPLIT is for config 5's 10^6 spheres.
BVH_REFERENCE, BVH_MEDIAN_SPLIT = 0, 1


def build():
    subprocess.run(["make", "-C", _HERE, "-s"], check=True)


def binding():
    """Bound oracle library (built on demand)."""
    global _binding
    if _binding is None:
        if not os.path.exists(_LIB):
            build()
        lib = C.CDLL(_LIB)
        b = abi.Binding(lib, "rto_", abi.BUILDER_FUNCS)
        b.add(_PROBES)
        _binding = b
    return _binding


def darr(*vals):
    a = np.array(vals, dtype=np.float64).ravel()
    return a, a.ctypes.data_as(_dp)


def render(scene, cam, params, n_threads=0, want_rgba8=True):
    """rto_render -> (linear HxWx3 float64, rgba8 HxWx4 uint8 or None, Stats)."""
    b = binding()
    h, w = params.height, params.width
    lin = np.zeros((h, w, 3), dtype=np.float64)
    rgba = np.zeros((h, w, 4), dtype=np.uint8) if want_rgba8 else None
    st = Stats()
    rc = b.render(scene.handle, C.byref(cam), C.byref(params), lin.ctypes.data,
                  rgba.ctypes.data if rgba is not None else None, C.byref(st), int(n_threads))
    abi.check(rc, b, "rto_render")
    return lin, rgba, st


def render_window(scene, cam, params, x0, y0, x1, y1, n_threads=0, want_var=False):
    """rto_render_window: the pixels [x0, x1) x [y0, y1) of the params.width x params.height render (same keys as the
    full image) -> (linear hxwx3, rgba8 hxwx4, per-channel variance of the sample radiances hxwx3 or None, Stats)."""
    b = binding()
    h, w = y1 - y0, x1 - x0
    lin = np.zeros((h, w, 3), dtype=np.float64)
    rgba = np.zeros((h, w, 4), dtype=np.uint8)
    var = np.zeros((h, w, 3), dtype=np.float64) if want_var else None
    st = Stats()
    rc = b.render_window(scene.handle, C.byref(cam), C.byref(params), x0, y0, x1, y1, lin.ctypes.data, rgba.ctypes.data,
                         var.ctypes.data if var is not None else None, C.byref(st), int(n_threads))
    abi.check(rc, b, "rto_render_window")
    return lin, rgba, var, st


def render_pixel_list(scene, cam, params, xs, ys, n_threads=0, want_var=False):
    """rto_render_pixel_list: the pixels (xs[k], ys[k]) of the full-size render -> (linear nx3, rgba8 nx4, variance nx3 or None)."""
    b = binding()
    xs = np.ascontiguousarray(xs, dtype=np.uint32)
    ys = np.ascontiguousarray(ys, dtype=np.uint32)
    n = len(xs)
    lin = np.zeros((n, 3), dtype=np.float64)
    rgba = np.zeros((n, 4), dtype=np.uint8)
    var = np.zeros((n, 3), dtype=np.float64) if want_var else None
    rc = b.render_pixel_list(scene.handle, C.byref(cam), C.byref(params), xs.ctypes.data, ys.ctypes.data, n, lin.ctypes.data,
                             rgba.ctypes.data, var.ctypes.data if var is not None else None, None, int(n_threads))
    abi.check(rc, b, "rto_render_pixel_list")
    return lin, rgba, var


PROBE_STRIDE = 12


def probe_path(scene, cam, params, px, row, sample, max_out=64):
    """rto_probe_path -> array [n_hits, 12]: t, p(3), normal(3), material id, u, v, front_face, scattered."""
    b = binding()
    out = np.zeros((max_out, PROBE_STRIDE), dtype=np.float64)
    n = b.probe_path(scene.handle, C.byref(cam), C.byref(params), px, row, sample, out.ctypes.data_as(_dp), max_out)
    abi.check(n, b, "rto_probe_path")
    return out[:n]


# ---- direct calls of one operation at a given input (the re-anchored per-bounce checker, tests/util.py)
DBL_MAX = float(np.finfo(np.float64).max)
SLOT_JITTER_U, SLOT_JITTER_V, SLOT_MEDIUM, SLOT_DIELECTRIC, SLOT_SCATTER = 0, 1, 0, 16, 32


def probe_camera_ray(cam, s, t, seed, pixel, sample):
    """rto_probe_camera_ray: Camera::ray(s, t) with the keyed draws of (seed, pixel, sample) -> [7] origin, direction, time."""
    out = np.zeros(7)
    abi.check(binding().probe_camera_ray(C.byref(cam), float(s), float(t), seed, pixel, sample, out.ctypes.data_as(_dp)),
              binding(), "rto_probe_camera_ray")
    return out


def probe_hit(scene, ray, t_min, seed, pixel, sample, bounce, quirks, t_max=DBL_MAX, world=-1):
    """rto_probe_hit: world.hit() (or any hittable's) for the ray [7] with the keyed draws of bounce `bounce` -> None on a
    miss, else [11] t, p(3), normal(3), u, v, front_face, material id."""
    ray = np.ascontiguousarray(ray, dtype=np.float64)
    out = np.zeros(11)
    rc = binding().probe_hit(scene.handle, world, ray.ctypes.data_as(_dp), float(t_min), float(t_max), seed, pixel, sample,
                             bounce, quirks, out.ctypes.data_as(_dp))
    abi.check(rc, binding(), "rto_probe_hit")
    return out if rc == 1 else None


def probe_scatter(scene, mat, ray, rec, seed, pixel, sample, bounce):
    """rto_probe_scatter: Material::scatter + emitted of material `mat` for the ray [7] and the record [10] (t, p, normal, u, v,
    front_face) -> [13] scattered (0/1), attenuation(3), scattered origin(3), direction(3), emitted(3)."""
    ray = np.ascontiguousarray(ray, dtype=np.float64)
    rec = np.ascontiguousarray(rec, dtype=np.float64)
    out = np.zeros(13)
    abi.check(binding().probe_scatter(scene.handle, mat, ray.ctypes.data_as(_dp), rec.ctypes.data_as(_dp), seed, pixel, sample,
                                      bounce, out.ctypes.data_as(_dp)), binding(), "rto_probe_scatter")
    return out


def probe_uniform(seed, pixel, sample, block, slot):
    return binding().probe_uniform(seed, pixel, sample, block, slot)


def probe_word(seed, pixel, sample, block, slot):
    return binding().probe_word(seed, pixel, sample, block, slot)


def probe_schlick(cosine, ri):
    return binding().probe_schlick(float(cosine), float(ri))
