"""Render drivers over the C ABI: the `render()` of the reference's main.rs:58-233, minus PNG/progress.

PyTorch is plumbing here (device buffers, the current HIP stream, torch.distributed over RCCL);
all tracing happens in the hand-written HIP kernels behind `rttnw_render_tiles_device`.
"""
import copy
import ctypes as C
import functools

import numpy as np

from . import abi, library, tiles
from .abi import Stats, check


def render_host(scene, cam, params, want_stats=True):
    """Blocking single-GPU render with host outputs: (linear HxWx3 f64, rgba8 HxWx4 u8, Stats)."""
    b = library.product()
    h, w = params.height, params.width
    lin = np.zeros((h, w, 3), dtype=np.float64)
    rgba = np.zeros((h, w, 4), dtype=np.uint8)
    st = Stats()
    rc = b.render(scene.handle, C.byref(cam), C.byref(params), lin.ctypes.data, rgba.ctypes.data,
                  C.byref(st) if want_stats else None)
    check(rc, b, "rttnw_render")
    return lin, rgba, st


def render_multi(scene, cam, params, device_ids, want_stats=True):
    """`rttnw_render_multi`: one call, the GPUs (or logical ranks) of `device_ids`; (linear, rgba8, [Stats per rank])."""
    b = library.product()
    h, w = params.height, params.width
    lin = np.zeros((h, w, 3), dtype=np.float64)
    rgba = np.zeros((h, w, 4), dtype=np.uint8)
    n = len(device_ids)
    ids = (C.c_int32 * n)(*device_ids)
    st = (Stats * n)()
    rc = b.render_multi(scene.handle, C.byref(cam), C.byref(params), n, ids, lin.ctypes.data, rgba.ctypes.data,
                        C.cast(st, C.c_void_p) if want_stats else None)
    check(rc, b, "rttnw_render_multi")
    return lin, rgba, list(st)


def _pass_params(params, pass_spp):
    """A copy of `params` — the caller's is never written to — with the adaptive drivers' default for a `spp_chunk` of 0: max(1, pass_spp // 16),
    so that a pass of 16 k samples is exactly one job group of 16 chunks (64 -> 4)."""
    p = copy.copy(params)
    if p.spp_chunk == 0:
        p.spp_chunk = max(1, pass_spp // 16)
    return p


def _frame_outputs(h, w):
    """Zeroed (linear hxwx3 f64, rgba8 hxwx4 u8, spp_map hxw u32, stderr hxwx3 f64)."""
    return (np.zeros((h, w, 3), dtype=np.float64), np.zeros((h, w, 4), dtype=np.uint8), np.zeros((h, w), dtype=np.uint32),
            np.zeros((h, w, 3), dtype=np.float64))


def _state_arrays(b, who, p, state, want_state):
    """(state_in, state_out) of the frame of `p`, either of them None: `state` as contiguous doubles of the right count — a ValueError in the name of
    `who` otherwise — and a zeroed array for the call to fill."""
    n_doubles = int(b.adaptive_state_doubles(p.width, p.height))
    st_in = None
    if state is not None:
        st_in = np.ascontiguousarray(state, dtype=np.float64).reshape(-1)
        if st_in.size != n_doubles:
            raise ValueError("%s: a state of a %dx%d frame holds %d doubles, got %d" % (who, p.width, p.height, n_doubles, st_in.size))
    return st_in, (np.zeros(n_doubles, dtype=np.float64) if want_state else None)


def _rank_args(device_ids):
    """(ngpu, device_ids, stats) as the node-wide entry points take them; None is the single form: ngpu 0, no ids, one Stats."""
    n = 0 if device_ids is None else len(device_ids)
    ids = None if device_ids is None else (C.c_int32 * max(n, 1))(*device_ids)
    return n, ids, (Stats * max(n, 1))()


def _denoise_params(iterations, sigma_luminance, sigma_normal, sigma_depth):
    return abi.Denoise(iterations=iterations, reserved0=0, sigma_luminance=sigma_luminance, sigma_normal=sigma_normal, sigma_depth=sigma_depth)


def _feature_arrays(features, h, w):
    """`render_features`' dict as contiguous f64 arrays of an hxw frame."""
    f = {k: np.ascontiguousarray(features[k], dtype=np.float64) for k in ("albedo", "normal", "depth", "alpha")}
    assert f["albedo"].shape == (h, w, 3) and f["normal"].shape == (h, w, 3) and f["depth"].shape == (h, w) and f["alpha"].shape == (h, w)
    return f


def _mask_array(who, mask, h, w):
    """`mask` as hxw bytes of 0 and 1, or None; a ValueError in the name of `who` for another shape."""
    if mask is None:
        return None
    m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
    if m.shape != (h, w):
        raise ValueError("%s: the mask must be (y1 - y0) x (x1 - x0) = %d x %d, got %s" % (who, h, w, m.shape))
    return m


def _ptr(a):
    return None if a is None else a.ctypes.data


def render_adaptive(scene, cam, params, pass_spp=64, rel_error=0.02, abs_error=0.0):
    """`rttnw_render_adaptive`: passes of `pass_spp` samples per pixel, a pixel stopping once its standard error is at most
    abs_error + rel_error * mean in every channel, or at `params.spp` samples (the cap, a multiple of pass_spp).  A `params.spp_chunk`
    of 0 is taken as max(1, pass_spp // 16) here, so that a pass of 16 k samples is exactly one job group of 16 chunks (64 -> 4).
    Returns (linear HxWx3 f64, rgba8 HxWx4 u8, spp_map HxW u32, stderr HxWx3 f64, Stats)."""
    b = library.product()
    p = _pass_params(params, pass_spp)
    lin, rgba, spp, se = _frame_outputs(p.height, p.width)
    st = Stats()
    a = abi.Adaptive(pass_spp=pass_spp, reserved0=0, rel_error=rel_error, abs_error=abs_error)
    rc = b.render_adaptive(scene.handle, C.byref(cam), C.byref(p), C.byref(a), lin.ctypes.data, rgba.ctypes.data, spp.ctypes.data,
                           se.ctypes.data, C.byref(st))
    check(rc, b, "rttnw_render_adaptive")
    return lin, rgba, spp, se, st


def render_adaptive_multi(scene, cam, params, device_ids, pass_spp=64, rel_error=0.02, abs_error=0.0):
    """`rttnw_render_adaptive_multi`: `render_adaptive` over the GPUs (or logical ranks) of `device_ids`, bit-identical outputs; the same
    `spp_chunk` default.  Returns (linear HxWx3 f64, rgba8 HxWx4 u8, spp_map HxW u32, stderr HxWx3 f64, [Stats per rank])."""
    b = library.product()
    p = _pass_params(params, pass_spp)
    lin, rgba, spp, se = _frame_outputs(p.height, p.width)
    n, ids, st = _rank_args(device_ids)
    a = abi.Adaptive(pass_spp=pass_spp, reserved0=0, rel_error=rel_error, abs_error=abs_error)
    rc = b.render_adaptive_multi(scene.handle, C.byref(cam), C.byref(p), C.byref(a), n, ids, lin.ctypes.data, rgba.ctypes.data,
                                 spp.ctypes.data, se.ctypes.data, C.cast(st, C.c_void_p))
    check(rc, b, "rttnw_render_adaptive_multi")
    return lin, rgba, spp, se, list(st)


def render_adaptive_resume(scene, cam, params, state=None, device_ids=None, pass_spp=64, rel_error=0.02, abs_error=0.0, want_state=True):
    """`rttnw_render_adaptive_resume`: `render_adaptive` (device_ids None) or `render_adaptive_multi` begun from `state` — the double array an
    earlier call returned, None for a fresh render — and continued under THIS call's tolerances and cap; the same `spp_chunk` default.  With a
    cap and tolerances no looser than the state's, the result is bit for bit the render that was never interrupted.
    Returns (linear HxWx3 f64, rgba8 HxWx4 u8, spp_map HxW u32, stderr HxWx3 f64, Stats or [Stats per rank], state or None)."""
    b = library.product()
    p = _pass_params(params, pass_spp)
    lin, rgba, spp, se = _frame_outputs(p.height, p.width)
    st_in, st_out = _state_arrays(b, "render_adaptive_resume", p, state, want_state)
    n, ids, st = _rank_args(device_ids)
    a = abi.Adaptive(pass_spp=pass_spp, reserved0=0, rel_error=rel_error, abs_error=abs_error)
    rc = b.render_adaptive_resume(scene.handle, C.byref(cam), C.byref(p), C.byref(a), n, ids, _ptr(st_in), _ptr(st_out), lin.ctypes.data,
                                  rgba.ctypes.data, spp.ctypes.data, se.ctypes.data, C.cast(st, C.c_void_p))
    check(rc, b, "rttnw_render_adaptive_resume")
    return lin, rgba, spp, se, (st[0] if device_ids is None else list(st)), st_out


def render_adaptive_region(scene, cam, params, x0, y0, x1, y1, mask=None, state=None, device_ids=None, pass_spp=64, rel_error=0.02, abs_error=0.0,
                           want_state=True):
    """`rttnw_render_adaptive_region`: `render_adaptive_resume` over the pixels [x0, x1) x [y0, y1) of the frame — all of them, or those whose byte
    of `mask` ((y1-y0) x (x1-x0), nonzero = selected) is set.  `state` is the frame-sized array an earlier call of this function or of
    `render_adaptive_resume` returned, in which a pixel never sampled is a record of zeros; None stands for all zeros.  Only selected pixels are
    traced, each to the bits a fresh whole-frame adaptive render under this cap and these tolerances gives it; the others keep their records.
    The same `spp_chunk` default.  Returns (linear hxwx3 f64, rgba8 hxwx4 u8, spp_map hxw u32, stderr hxwx3 f64, Stats or [Stats per rank],
    state or None), h = y1 - y0, w = x1 - x0; a pixel of the window without samples is zero everywhere, alpha included."""
    b = library.product()
    p = _pass_params(params, pass_spp)
    h, w = max(int(y1) - int(y0), 0), max(int(x1) - int(x0), 0)
    m = _mask_array("render_adaptive_region", mask, h, w)
    lin, rgba, spp, se = _frame_outputs(h, w)
    st_in, st_out = _state_arrays(b, "render_adaptive_region", p, state, want_state)
    n, ids, st = _rank_args(device_ids)
    a = abi.Adaptive(pass_spp=pass_spp, reserved0=0, rel_error=rel_error, abs_error=abs_error)
    rc = b.render_adaptive_region(scene.handle, C.byref(cam), C.byref(p), C.byref(a), x0, y0, x1, y1, _ptr(m), n, ids, _ptr(st_in), _ptr(st_out),
                                  lin.ctypes.data, rgba.ctypes.data, spp.ctypes.data, se.ctypes.data, C.cast(st, C.c_void_p))
    check(rc, b, "rttnw_render_adaptive_region")
    return lin, rgba, spp, se, (st[0] if device_ids is None else list(st)), st_out


def render_adaptive_denoised(scene, cam, params, pass_spp=64, rel_error=0.02, abs_error=0.0, iterations=5, feature_spp=0, sigma_luminance=0.0,
                             sigma_normal=0.0, sigma_depth=0.0, want_state=True):
    """`rttnw_render_adaptive_denoised`: adaptive rounds of `pass_spp` samples whose stopping rule reads the FILTERED image — after every round
    the frame goes through `denoise`'s passes on the device (features of `feature_spp` samples, 0 = pass_spp) and a pixel stops once
    sqrt(filtered variance) <= abs_error + rel_error * filtered value in every channel, or at `params.spp` samples.  The same `spp_chunk`
    default as `render_adaptive`.  Returns a dict: "linear" HxWx3 f64 and "rgba8" HxWx4 u8 (the denoised image), "spp" HxW u32, "stderr" HxWx3
    f64 (sqrt of the filtered variance), "raw_linear" and "raw_stderr" HxWx3 f64 (`render_adaptive`'s values), "state" (what
    `render_adaptive_resume` takes, or None), "rounds" (rounds run) and "stats"."""
    b = library.product()
    p = _pass_params(params, pass_spp)
    h, w = p.height, p.width
    out = {"linear": np.zeros((h, w, 3)), "rgba8": np.zeros((h, w, 4), dtype=np.uint8), "spp": np.zeros((h, w), dtype=np.uint32),
           "stderr": np.zeros((h, w, 3)), "raw_linear": np.zeros((h, w, 3)), "raw_stderr": np.zeros((h, w, 3))}
    _, state = _state_arrays(b, "render_adaptive_denoised", p, None, want_state)
    st = Stats()
    a = abi.Adaptive(pass_spp=pass_spp, reserved0=0, rel_error=rel_error, abs_error=abs_error)
    g = abi.Guided(feature_spp=feature_spp, reserved0=0, denoise=_denoise_params(iterations, sigma_luminance, sigma_normal, sigma_depth))
    rc = b.render_adaptive_denoised(scene.handle, C.byref(cam), C.byref(p), C.byref(a), C.byref(g), out["linear"].ctypes.data,
                                    out["rgba8"].ctypes.data, out["spp"].ctypes.data, out["stderr"].ctypes.data, out["raw_linear"].ctypes.data,
                                    out["raw_stderr"].ctypes.data, _ptr(state), C.byref(st))
    check(rc, b, "rttnw_render_adaptive_denoised")
    out["state"] = state
    out["rounds"] = int(out["spp"].max()) // pass_spp  # (every round traces its active pixels: the pixel that went furthest took part in all)
    out["stats"] = st
    return out


def render_features(scene, cam, params):
    """`rttnw_render_features`: the first hit of the render's own camera rays, averaged over `params.spp` samples per pixel.
    Returns {"albedo": HxWx3, "normal": HxWx3, "depth": HxW, "alpha": HxW (all f64), "stats": Stats}."""
    b = library.product()
    h, w = params.height, params.width
    out = {"albedo": np.zeros((h, w, 3)), "normal": np.zeros((h, w, 3)), "depth": np.zeros((h, w)), "alpha": np.zeros((h, w))}
    st = Stats()
    rc = b.render_features(scene.handle, C.byref(cam), C.byref(params), out["albedo"].ctypes.data, out["normal"].ctypes.data,
                           out["depth"].ctypes.data, out["alpha"].ctypes.data, C.byref(st))
    check(rc, b, "rttnw_render_features")
    out["stats"] = st
    return out


def render_region(scene, cam, params, x0, y0, x1, y1, mask=None):
    """`rttnw_render_region`: pixels [x0, x1) x [y0, y1) of the frame `render_host` renders — all of them, or those whose byte of
    `mask` ((y1-y0) x (x1-x0), nonzero = selected) is set — each bit-identical to the full render's; an unselected pixel comes back as
    0, 0, 0 with alpha 0.  Returns (linear hxwx3 f64, rgba8 hxwx4 u8, Stats), h = y1 - y0, w = x1 - x0."""
    b = library.product()
    h, w = max(int(y1) - int(y0), 0), max(int(x1) - int(x0), 0)
    m = _mask_array("render_region", mask, h, w)
    lin, rgba, _, _ = _frame_outputs(h, w)
    st = Stats()
    rc = b.render_region(scene.handle, C.byref(cam), C.byref(params), x0, y0, x1, y1, _ptr(m), lin.ctypes.data, rgba.ctypes.data, C.byref(st))
    check(rc, b, "rttnw_render_region")
    return lin, rgba, st


def denoise(linear, features, stderr=None, iterations=5, sigma_luminance=0.0, sigma_normal=0.0, sigma_depth=0.0, want_ms=False, variance=None):
    """`rttnw_denoise`: the edge-avoiding a-trous filter over `linear` (HxWx3), guided by `features` (what `render_features` returns)
    and, when `stderr` (HxWx3, `render_adaptive`'s standard errors of the pixel means) is given, by their variance — or by `variance` (HxWx3, in
    place of `stderr`: the variance of the pixel means as it stands, `temporal_variance`'s for one).  A sigma of 0 is
    the library default.  Returns (linear HxWx3 f64, rgba8 HxWx4 u8, variance HxWx3 f64 or None) — and the device time in ms after
    them with `want_ms`."""
    b = library.product()
    lin = np.ascontiguousarray(linear, dtype=np.float64)
    h, w = lin.shape[:2]
    if stderr is not None and variance is not None:
        raise ValueError("denoise: stderr or variance, not both")
    var = None if stderr is None else np.ascontiguousarray(np.square(np.asarray(stderr, dtype=np.float64)))
    if variance is not None:
        var = np.ascontiguousarray(variance, dtype=np.float64)
    f = _feature_arrays(features, h, w)
    assert var is None or var.shape == (h, w, 3)
    out = np.zeros((h, w, 3))
    rgba = np.zeros((h, w, 4), dtype=np.uint8)
    out_var = None if var is None else np.zeros((h, w, 3))
    d = _denoise_params(iterations, sigma_luminance, sigma_normal, sigma_depth)
    ms = C.c_double(0.0)
    rc = b.denoise(w, h, lin.ctypes.data, _ptr(var), f["albedo"].ctypes.data, f["normal"].ctypes.data, f["depth"].ctypes.data,
                   f["alpha"].ctypes.data, C.byref(d), out.ctypes.data, rgba.ctypes.data, _ptr(out_var), C.byref(ms))
    check(rc, b, "rttnw_denoise")
    return (out, rgba, out_var, ms.value) if want_ms else (out, rgba, out_var)


def render_halves(scene, cam, params):
    """The two half-buffers `denoise_nlm` takes: two `render_host` calls of `params.spp // 2` samples each, at `sample_begin` and
    `sample_begin + spp // 2` — disjoint sample ranges, so their mean is the render of `params.spp` samples up to rounding.  An odd spp is a
    ValueError.  Returns ((linear_a, rgba8_a, Stats_a), (linear_b, rgba8_b, Stats_b))."""
    if params.spp < 2 or params.spp % 2:
        raise ValueError("render_halves: spp must be even and at least 2 (two halves of spp // 2 samples), got %d" % params.spp)
    halves = []
    for k in range(2):
        p = copy.copy(params)
        p.spp = params.spp // 2
        p.sample_begin = params.sample_begin + k * p.spp
        halves.append(render_host(scene, cam, p))
    return tuple(halves)


def denoise_nlm(half_a, half_b, var_a=None, var_b=None, search_radius=0, patch_radius=0, k=0.0, want_ms=False):
    """`rttnw_denoise_nlm`: non-local means over two half-buffers (HxWx3 each, the means of two disjoint, equally large sample sets — what
    `render_halves` returns): the weights that average one half are patch distances measured in the other.  No feature buffer.  `var_a`, `var_b`
    (HxWx3, both or neither) are the variances of each half's pixel means — the square of `render_adaptive`'s stderr of that half; without them
    the filter estimates one from the difference of the halves.  A parameter of 0 is the library default (search radius 7, patch radius 3,
    k 0.7).  Returns a dict: "linear" HxWx3 f64 and "rgba8" HxWx4 u8 (the filtered image), "half_a" and "half_b" HxWx3 (the two cross-filtered
    halves), "error" HxWx3 ((a' - b')^2 / 4) — and "ms", the device time, with `want_ms`."""
    b = library.product()
    a_, b_ = np.ascontiguousarray(half_a, dtype=np.float64), np.ascontiguousarray(half_b, dtype=np.float64)
    h, w = a_.shape[:2]
    if (var_a is None) != (var_b is None):
        raise ValueError("denoise_nlm: var_a and var_b go together: both or neither")
    va = None if var_a is None else np.ascontiguousarray(var_a, dtype=np.float64)
    vb = None if var_b is None else np.ascontiguousarray(var_b, dtype=np.float64)
    for arr in (a_, b_, va, vb):
        if arr is not None and arr.shape != (h, w, 3):
            raise ValueError("denoise_nlm: every input is HxWx3 of one frame, got %s beside %s" % (arr.shape, (h, w, 3)))
    out = {"linear": np.zeros((h, w, 3)), "rgba8": np.zeros((h, w, 4), dtype=np.uint8), "half_a": np.zeros((h, w, 3)),
           "half_b": np.zeros((h, w, 3)), "error": np.zeros((h, w, 3))}
    d = abi.Nlm(search_radius=search_radius, patch_radius=patch_radius, k=k, reserved0=0, reserved1=0)
    ms = C.c_double(0.0)
    rc = b.denoise_nlm(w, h, a_.ctypes.data, b_.ctypes.data, _ptr(va), _ptr(vb), C.byref(d), out["linear"].ctypes.data, out["rgba8"].ctypes.data,
                       out["half_a"].ctypes.data, out["half_b"].ctypes.data, out["error"].ctypes.data, C.byref(ms))
    check(rc, b, "rttnw_denoise_nlm")
    if want_ms:
        out["ms"] = ms.value
    return out


REGRESS_OUTPUTS = ("linear", "rgba8", "half_a", "half_b", "error", "fit")


def denoise_regress(half_a, half_b, var_a=None, var_b=None, features=None, *, mask=7, demodulate=True, ridge=0.0, search_radius=0, patch_radius=0,
                    k=0.0, want_ms=False):
    """`rttnw_denoise_regress`: first-order regression of colour on the first-hit features, weighted by `denoise_nlm`'s cross-filtered weights,
    over the two half-buffers `render_halves` returns.  `features` is what `render_features` returns (it may be None with `mask` 0 and
    `demodulate` False: the call is then `denoise_nlm`, bit for bit); `mask` selects the regressors (bits: 1 albedo, 2 normal, 4 depth),
    `demodulate` filters colour / albedo, `ridge` 0 is the library default; the other parameters are `denoise_nlm`'s.  Returns `denoise_nlm`'s dict
    plus "fit" HxW (0, 1 or 2: how many of the two directions used the first-order value) — and "ms", the device time, with `want_ms`."""
    b = library.product()
    a_, b_ = np.ascontiguousarray(half_a, dtype=np.float64), np.ascontiguousarray(half_b, dtype=np.float64)
    h, w = a_.shape[:2]
    if (var_a is None) != (var_b is None):
        raise ValueError("denoise_regress: var_a and var_b go together: both or neither")
    va = None if var_a is None else np.ascontiguousarray(var_a, dtype=np.float64)
    vb = None if var_b is None else np.ascontiguousarray(var_b, dtype=np.float64)
    for arr in (a_, b_, va, vb):
        if arr is not None and arr.shape != (h, w, 3):
            raise ValueError("denoise_regress: every half and variance is HxWx3 of one frame, got %s beside %s" % (arr.shape, (h, w, 3)))
    if not 0 <= int(mask) <= 7:
        raise ValueError("denoise_regress: mask must be 0 .. 7 (bits: 1 albedo, 2 normal, 4 depth), got %r" % (mask,))
    if not ridge >= 0.0:
        raise ValueError("denoise_regress: ridge must be at least 0 (0: the library default), got %r" % (ridge,))
    if features is None and (mask or demodulate):
        raise ValueError("denoise_regress: a mask other than 0 and demodulate need features (what render_features returns)")
    f = {name: None for name in ("albedo", "normal", "depth", "alpha")} if features is None else _feature_arrays(features, h, w)
    out = {"linear": np.zeros((h, w, 3)), "rgba8": np.zeros((h, w, 4), dtype=np.uint8), "half_a": np.zeros((h, w, 3)),
           "half_b": np.zeros((h, w, 3)), "error": np.zeros((h, w, 3)), "fit": np.zeros((h, w))}
    g = abi.Regress(search_radius=search_radius, patch_radius=patch_radius, k=k, ridge=ridge, features=int(mask), demodulate=1 if demodulate else 0,
                    reserved0=0, reserved1=0)
    ms = C.c_double(0.0)
    rc = b.denoise_regress(w, h, a_.ctypes.data, b_.ctypes.data, _ptr(va), _ptr(vb), _ptr(f["albedo"]), _ptr(f["normal"]), _ptr(f["depth"]),
                           _ptr(f["alpha"]), C.byref(g), *[out[name].ctypes.data for name in REGRESS_OUTPUTS], C.byref(ms))
    check(rc, b, "rttnw_denoise_regress")
    if want_ms:
        out["ms"] = ms.value
    return out


SELECT_OUTPUTS = ("linear", "rgba8", "blend", "feature", "nlm", "error")


def denoise_select(half_a, half_b, features, var_a=None, var_b=None, iterations=5, sigma_luminance=0.0, sigma_normal=0.0, sigma_depth=0.0,
                   search_radius=0, patch_radius=0, k=0.0, error_radius=0, blend_radius=0, margin=None, want_ms=False):
    """`rttnw_denoise_select`: per pixel, the better of `denoise` (guided by `features`, what `render_features` returns) and `denoise_nlm` over
    the two half-buffers `render_halves` returns.  Each half is filtered by both; a filtered half is scored against the other, raw half, the
    normalised error difference is summed over (2 error_radius + 1)^2 pixels, non-local means is chosen where its mean exceeds `margin`, and the
    choice is averaged over (2 blend_radius + 1)^2 pixels into the blend weight.  `var_a`, `var_b` (HxWx3, both or neither): the variances of
    each half's pixel means, given to both filters.  `margin` None is the library default (0.01); a margin of 0 is a margin of 0.  The other
    parameters are the two filters' own.  Returns a dict: "linear" HxWx3 f64 and "rgba8" HxWx4 u8 (the blended image), "blend" HxW (the weight
    of non-local means, 0 .. 1), "feature" and "nlm" HxWx3 (the mean of each filter's two filtered halves), "error" HxWx3 — and "ms", the
    device time, with `want_ms`."""
    b = library.product()
    a_, b_ = np.ascontiguousarray(half_a, dtype=np.float64), np.ascontiguousarray(half_b, dtype=np.float64)
    h, w = a_.shape[:2]
    if (var_a is None) != (var_b is None):
        raise ValueError("denoise_select: var_a and var_b go together: both or neither")
    va = None if var_a is None else np.ascontiguousarray(var_a, dtype=np.float64)
    vb = None if var_b is None else np.ascontiguousarray(var_b, dtype=np.float64)
    for arr in (a_, b_, va, vb):
        if arr is not None and arr.shape != (h, w, 3):
            raise ValueError("denoise_select: every half and variance is HxWx3 of one frame, got %s beside %s" % (arr.shape, (h, w, 3)))
    if margin is not None and not -2.0 <= margin <= 2.0:
        raise ValueError("denoise_select: margin must lie in [-2, 2] (None: the default, 0.01), got %r" % (margin,))
    f = _feature_arrays(features, h, w)
    out = {"linear": np.zeros((h, w, 3)), "rgba8": np.zeros((h, w, 4), dtype=np.uint8), "blend": np.zeros((h, w)), "feature": np.zeros((h, w, 3)),
           "nlm": np.zeros((h, w, 3)), "error": np.zeros((h, w, 3))}
    dn = _denoise_params(iterations, sigma_luminance, sigma_normal, sigma_depth)
    nl = abi.Nlm(search_radius=search_radius, patch_radius=patch_radius, k=k, reserved0=0, reserved1=0)
    sel = abi.Select(error_radius=error_radius, blend_radius=blend_radius, margin=0.0 if margin is None else margin,
                     use_default_margin=1 if margin is None else 0, reserved0=0)
    ms = C.c_double(0.0)
    rc = b.denoise_select(w, h, a_.ctypes.data, b_.ctypes.data, _ptr(va), _ptr(vb), f["albedo"].ctypes.data, f["normal"].ctypes.data,
                          f["depth"].ctypes.data, f["alpha"].ctypes.data, C.byref(dn), C.byref(nl), C.byref(sel),
                          *[out[name].ctypes.data for name in SELECT_OUTPUTS], C.byref(ms))
    check(rc, b, "rttnw_denoise_select")
    if want_ms:
        out["ms"] = ms.value
    return out


TEMPORAL_OUTPUTS = ("linear", "rgba8", "variance", "length", "prev_xy")


def _temporal_frame(who, linear, max_history, depth_tolerance, normal_min):
    """What `temporal_accumulate` and `temporal_variance` check first: the frame as a contiguous HxWx3 array, behind the three parameters' ranges."""
    lin = np.ascontiguousarray(linear, dtype=np.float64)
    if lin.ndim != 3 or lin.shape[2] != 3:
        raise ValueError("%s: the frame is HxWx3, got %s" % (who, lin.shape))
    if not 0 <= int(max_history) <= 65535:
        raise ValueError("%s: max_history must be 0 .. 65535 (0: the default, 32), got %r" % (who, max_history))
    if not depth_tolerance >= 0.0:
        raise ValueError("%s: depth_tolerance must be at least 0 (0: the default, 0.05), got %r" % (who, depth_tolerance))
    if not -1.0 <= normal_min <= 1.0:
        raise ValueError("%s: normal_min must lie in [-1, 1] (0: the default, 0.9; -1: no normal test), got %r" % (who, normal_min))
    return lin


def temporal_accumulate(linear, features, cam, history=None, variance=None, max_history=0, depth_tolerance=0.0, normal_min=0.0, want_ms=False):
    """`rttnw_temporal_accumulate`: this frame (`linear` HxWx3, its `features` as `render_features` returns them, its camera `cam`) blended with the
    previous call's result, which is fetched from where each pixel's surface point was in the previous frame, through four bilinear taps that
    are kept only where depth and normal say "same surface".  `history`: the dict a previous call returned (it carries that frame's features and
    camera), or None to start a sequence.  `variance` (HxWx3): the variance of this frame's pixel means; beside a history both frames have one or
    neither.  A parameter of 0 is the library default (32 frames, depth within 5 %, a normalised normal product of 0.9); `normal_min` -1 switches
    the normal test off.  Returns a dict: "linear" HxWx3 f64 and "rgba8" HxWx4 u8 (the accumulated image), "variance" HxWx3 or None, "length" HxW
    (the frames each pixel's history counts), "prev_xy" HxWx2 (where the pixel was in the previous frame; NaN without a history), "features" and
    "cam" as given — and "ms", the kernel's time, with `want_ms`."""
    who = "temporal_accumulate"
    lin = _temporal_frame(who, linear, max_history, depth_tolerance, normal_min)
    h, w = lin.shape[:2]
    var = None if variance is None else np.ascontiguousarray(variance, dtype=np.float64)
    prev = [None] * 6
    prev_cam = None
    if history is not None:
        missing = [k for k in ("linear", "length", "features", "cam") if history.get(k) is None]
        if missing:
            raise ValueError("%s: the history is a previous call's result (it lacks %s)" % (who, ", ".join(missing)))
        if (var is None) != (history.get("variance") is None):
            raise ValueError("%s: beside a history both frames have a variance or neither has" % who)
        pf = history["features"]
        prev = [None if a is None else np.ascontiguousarray(a, dtype=np.float64)
                for a in (history["linear"], history.get("variance"), history["length"], pf["normal"], pf["depth"], pf["alpha"])]
        prev_cam = history["cam"]
    f = {k: np.ascontiguousarray(features[k], dtype=np.float64) for k in ("normal", "depth", "alpha")}
    for arr, shape in ((var, (h, w, 3)), (f["normal"], (h, w, 3)), (f["depth"], (h, w)), (f["alpha"], (h, w)), (prev[0], (h, w, 3)), (prev[1], (h, w, 3)),
                       (prev[2], (h, w)), (prev[3], (h, w, 3)), (prev[4], (h, w)), (prev[5], (h, w))):
        if arr is not None and arr.shape != shape:
            raise ValueError("%s: every array is of one %dx%d frame, got %s where %s was expected" % (who, w, h, arr.shape, shape))
    b = library.product()
    out = {"linear": np.zeros((h, w, 3)), "rgba8": np.zeros((h, w, 4), dtype=np.uint8), "variance": None if var is None else np.zeros((h, w, 3)),
           "length": np.zeros((h, w)), "prev_xy": np.zeros((h, w, 2))}
    t = abi.Temporal(max_history=int(max_history), reserved0=0, depth_tolerance=depth_tolerance, normal_min=normal_min)
    ms = C.c_double(0.0)
    rc = b.temporal_accumulate(w, h, C.byref(cam), None if prev_cam is None else C.byref(prev_cam), lin.ctypes.data, _ptr(var), f["normal"].ctypes.data,
                               f["depth"].ctypes.data, f["alpha"].ctypes.data, *[_ptr(a) for a in prev], C.byref(t),
                               *[_ptr(out[name]) for name in TEMPORAL_OUTPUTS], C.byref(ms))
    check(rc, b, "rttnw_temporal_accumulate")
    out["features"], out["cam"] = features, cam
    if want_ms:
        out["ms"] = ms.value
    return out


VARIANCE_OUTPUTS = ("linear", "rgba8", "moment2", "length", "prev_xy", "variance")


def temporal_variance(linear, features, cam, history=None, min_temporal=0, radius=0, sigma_normal=0.0, sigma_depth=0.0, max_history=0,
                      depth_tolerance=0.0, normal_min=0.0, want_ms=False):
    """`rttnw_temporal_variance`: `temporal_accumulate` of this frame without variances, the second moment of the colour carried along the same
    reprojected history, and the variance of each pixel's accumulated mean read off the two moments — where the history counts at least
    `min_temporal` frames; elsewhere from a (2 radius + 1)^2 window of neighbours weighted by normal and depth as `denoise` weighs them
    (`sigma_normal`, `sigma_depth`).  `history`: the dict a previous call returned, or None to start a sequence.  A parameter of 0 is the library
    default (4 frames, radius 3, the filter's sigmas; `temporal_accumulate`'s for the other three).  Returns that function's dict with "moment2"
    HxWx3 in place of its "variance", and "variance" HxWx3: the variance of the pixel means, which `denoise` takes as its `variance`."""
    who = "temporal_variance"
    lin = _temporal_frame(who, linear, max_history, depth_tolerance, normal_min)
    h, w = lin.shape[:2]
    if int(min_temporal) == 1 or not 0 <= int(min_temporal) <= 65535:
        raise ValueError("%s: min_temporal must be 0 (the default, 4) or 2 .. 65535, got %r" % (who, min_temporal))
    if not 0 <= int(radius) <= 4:
        raise ValueError("%s: radius must be 0 .. 4 (0: the default, 3), got %r" % (who, radius))
    if not sigma_normal >= 0.0 or not sigma_depth >= 0.0:
        raise ValueError("%s: sigma_normal and sigma_depth must be at least 0 (0: the defaults, 64 and 0.1), got %r, %r" % (who, sigma_normal, sigma_depth))
    prev = [None] * 6
    prev_cam = None
    if history is not None:
        missing = [k for k in ("linear", "moment2", "length", "features", "cam") if history.get(k) is None]
        if missing:
            raise ValueError("%s: the history is a previous call's result (it lacks %s)" % (who, ", ".join(missing)))
        pf = history["features"]
        prev = [np.ascontiguousarray(a, dtype=np.float64) for a in (history["linear"], history["moment2"], history["length"], pf["normal"], pf["depth"],
                                                                    pf["alpha"])]
        prev_cam = history["cam"]
    f = {k: np.ascontiguousarray(features[k], dtype=np.float64) for k in ("normal", "depth", "alpha")}
    for arr, shape in ((f["normal"], (h, w, 3)), (f["depth"], (h, w)), (f["alpha"], (h, w)), (prev[0], (h, w, 3)), (prev[1], (h, w, 3)), (prev[2], (h, w)),
                       (prev[3], (h, w, 3)), (prev[4], (h, w)), (prev[5], (h, w))):
        if arr is not None and arr.shape != shape:
            raise ValueError("%s: every array is of one %dx%d frame, got %s where %s was expected" % (who, w, h, arr.shape, shape))
    b = library.product()
    out = {"linear": np.zeros((h, w, 3)), "rgba8": np.zeros((h, w, 4), dtype=np.uint8), "moment2": np.zeros((h, w, 3)), "length": np.zeros((h, w)),
           "prev_xy": np.zeros((h, w, 2)), "variance": np.zeros((h, w, 3))}
    t = abi.Temporal(max_history=int(max_history), reserved0=0, depth_tolerance=depth_tolerance, normal_min=normal_min)
    v = abi.Variance(min_temporal=int(min_temporal), radius=int(radius), sigma_normal=sigma_normal, sigma_depth=sigma_depth, reserved0=0, reserved1=0)
    ms = C.c_double(0.0)
    rc = b.temporal_variance(w, h, C.byref(cam), None if prev_cam is None else C.byref(prev_cam), lin.ctypes.data, f["normal"].ctypes.data,
                             f["depth"].ctypes.data, f["alpha"].ctypes.data, *[_ptr(a) for a in prev], C.byref(t), C.byref(v),
                             *[_ptr(out[name]) for name in VARIANCE_OUTPUTS], C.byref(ms))
    check(rc, b, "rttnw_temporal_variance")
    out["features"], out["cam"] = features, cam
    if want_ms:
        out["ms"] = ms.value
    return out


CLAMP_OUTPUTS = VARIANCE_OUTPUTS + ("mean", "sd", "clipped")


def _clamp_params(who, gamma, clamp_radius, clamp_sigma_normal, clamp_sigma_depth):
    """`rttnw_clamp_params` behind its ranges."""
    if not gamma >= 0.0:
        raise ValueError("%s: gamma must be at least 0 (0: the default, 1.0; inf: never clip), got %r" % (who, gamma))
    if not 0 <= int(clamp_radius) <= 4:
        raise ValueError("%s: clamp_radius must be 0 .. 4 (0: the default, 3), got %r" % (who, clamp_radius))
    if not clamp_sigma_normal >= 0.0 or not clamp_sigma_depth >= 0.0:
        raise ValueError("%s: clamp_sigma_normal and clamp_sigma_depth must be at least 0 (0: the defaults, 64 and 0.1), got %r, %r"
                         % (who, clamp_sigma_normal, clamp_sigma_depth))
    return abi.Clamp(radius=int(clamp_radius), reserved0=0, gamma=float(gamma), sigma_normal=clamp_sigma_normal, sigma_depth=clamp_sigma_depth)


def temporal_clamp(linear, features, cam, history=None, gamma=0.0, clamp_radius=0, clamp_sigma_normal=0.0, clamp_sigma_depth=0.0, min_temporal=0,
                   radius=0, sigma_normal=0.0, sigma_depth=0.0, max_history=0, depth_tolerance=0.0, normal_min=0.0, want_ms=False, want_statistics=True):
    """`rttnw_temporal_clamp`: `temporal_variance` with the reprojected history clipped to the frame in front of the blend — the mean and the
    standard deviation of THIS frame's colour over a (2 clamp_radius + 1)^2 window, weighted by normal and depth as the variance estimate's
    window is (`clamp_sigma_normal`, `clamp_sigma_depth`), admit the history inside mean +- `gamma` deviations and move it to the nearer bound
    outside.  A parameter of 0 is the library default (gamma 1, radius 3, the filter's sigmas); a gamma of inf never clips.  The other keywords
    are `temporal_variance`'s.  Returns that function's dict with "mean" and "sd" HxWx3 (the window's statistics) and "clipped" HxW u8 (bit ch: the
    channel was clipped), usable as the next call's history.  Without `want_statistics` "mean" and "sd" are not asked for (None): the kernel then
    takes the statistics only where a history is blended, as the `SvgfSequence` handle runs it."""
    who = "temporal_clamp"
    lin = _temporal_frame(who, linear, max_history, depth_tolerance, normal_min)
    h, w = lin.shape[:2]
    if int(min_temporal) == 1 or not 0 <= int(min_temporal) <= 65535:
        raise ValueError("%s: min_temporal must be 0 (the default, 4) or 2 .. 65535, got %r" % (who, min_temporal))
    if not 0 <= int(radius) <= 4:
        raise ValueError("%s: radius must be 0 .. 4 (0: the default, 3), got %r" % (who, radius))
    if not sigma_normal >= 0.0 or not sigma_depth >= 0.0:
        raise ValueError("%s: sigma_normal and sigma_depth must be at least 0 (0: the defaults, 64 and 0.1), got %r, %r" % (who, sigma_normal, sigma_depth))
    k = _clamp_params(who, gamma, clamp_radius, clamp_sigma_normal, clamp_sigma_depth)
    prev = [None] * 6
    prev_cam = None
    if history is not None:
        missing = [key for key in ("linear", "moment2", "length", "features", "cam") if history.get(key) is None]
        if missing:
            raise ValueError("%s: the history is a previous call's result (it lacks %s)" % (who, ", ".join(missing)))
        pf = history["features"]
        prev = [np.ascontiguousarray(a, dtype=np.float64) for a in (history["linear"], history["moment2"], history["length"], pf["normal"], pf["depth"],
                                                                    pf["alpha"])]
        prev_cam = history["cam"]
    f = {key: np.ascontiguousarray(features[key], dtype=np.float64) for key in ("normal", "depth", "alpha")}
    for arr, shape in ((f["normal"], (h, w, 3)), (f["depth"], (h, w)), (f["alpha"], (h, w)), (prev[0], (h, w, 3)), (prev[1], (h, w, 3)), (prev[2], (h, w)),
                       (prev[3], (h, w, 3)), (prev[4], (h, w)), (prev[5], (h, w))):
        if arr is not None and arr.shape != shape:
            raise ValueError("%s: every array is of one %dx%d frame, got %s where %s was expected" % (who, w, h, arr.shape, shape))
    b = library.product()
    out = {"linear": np.zeros((h, w, 3)), "rgba8": np.zeros((h, w, 4), dtype=np.uint8), "moment2": np.zeros((h, w, 3)), "length": np.zeros((h, w)),
           "prev_xy": np.zeros((h, w, 2)), "variance": np.zeros((h, w, 3)), "mean": np.zeros((h, w, 3)) if want_statistics else None,
           "sd": np.zeros((h, w, 3)) if want_statistics else None, "clipped": np.zeros((h, w), dtype=np.uint8)}
    t = abi.Temporal(max_history=int(max_history), reserved0=0, depth_tolerance=depth_tolerance, normal_min=normal_min)
    v = abi.Variance(min_temporal=int(min_temporal), radius=int(radius), sigma_normal=sigma_normal, sigma_depth=sigma_depth, reserved0=0, reserved1=0)
    ms = C.c_double(0.0)
    rc = b.temporal_clamp(w, h, C.byref(cam), None if prev_cam is None else C.byref(prev_cam), lin.ctypes.data, f["normal"].ctypes.data,
                          f["depth"].ctypes.data, f["alpha"].ctypes.data, *[_ptr(a) for a in prev], C.byref(t), C.byref(v), C.byref(k),
                          *[_ptr(out[name]) for name in CLAMP_OUTPUTS], C.byref(ms))
    check(rc, b, "rttnw_temporal_clamp")
    out["features"], out["cam"] = features, cam
    if want_ms:
        out["ms"] = ms.value
    return out


PROBE_OUTPUTS = ("length", "prev_xy", "multiplier")


def _sampling_params(who, boost, fill):
    """`rttnw_sampling_params` behind its ranges."""
    if int(boost) not in (0, 1, 2, 4, 8):
        raise ValueError("%s: boost must be 1, 2, 4 or 8 (0: the default, 8), got %r" % (who, boost))
    if not (fill == 0.0 or 1.0 <= fill < float("inf")):
        raise ValueError("%s: fill must be finite and at least 1 (0: the default, 8.0), got %r" % (who, fill))
    return abi.Sampling(boost=int(boost), reserved0=0, fill=float(fill))


def temporal_probe(features, cam, history=None, boost=0, fill=0.0, max_history=0, depth_tolerance=0.0, normal_min=0.0, want_ms=False):
    """`rttnw_temporal_probe`: where each pixel's history is and how long, from the frame's `features` and camera and the previous call's result
    alone — no colour —, and how many times the frame's samples the pixel should get: the largest of 1, 2, 4, 8 that is at most `boost` and at
    most floor(`fill` / (length + 1)); 1 on a miss.  `history`: a dict with "length", "features" and "cam" (what `temporal_accumulate` and its
    kin return), or None: no history, every hit pixel gets the first frame's multiplier.  A parameter of 0 is the library default (boost 8,
    fill 8.0, `temporal_accumulate`'s three).  Returns a dict: "length" HxW (the reprojected history length, 0 where there is none), "prev_xy"
    HxWx2 (`temporal_accumulate`'s), "multiplier" HxW u8 — and "ms", the kernel's time, with `want_ms`."""
    who = "temporal_probe"
    f = {k: np.ascontiguousarray(features[k], dtype=np.float64) for k in ("normal", "depth", "alpha")}
    if f["depth"].ndim != 2:
        raise ValueError("%s: the depth map is HxW, got %s" % (who, f["depth"].shape))
    h, w = f["depth"].shape
    _temporal_frame(who, np.zeros((1, 1, 3)), max_history, depth_tolerance, normal_min)
    a = _sampling_params(who, boost, fill)
    prev = [None] * 4
    prev_cam = None
    if history is not None:
        missing = [k for k in ("length", "features", "cam") if history.get(k) is None]
        if missing:
            raise ValueError("%s: the history is a previous call's result (it lacks %s)" % (who, ", ".join(missing)))
        pf = history["features"]
        prev = [np.ascontiguousarray(x, dtype=np.float64) for x in (history["length"], pf["normal"], pf["depth"], pf["alpha"])]
        prev_cam = history["cam"]
    for arr, shape in ((f["normal"], (h, w, 3)), (f["alpha"], (h, w)), (prev[0], (h, w)), (prev[1], (h, w, 3)), (prev[2], (h, w)), (prev[3], (h, w))):
        if arr is not None and arr.shape != shape:
            raise ValueError("%s: every array is of one %dx%d frame, got %s where %s was expected" % (who, w, h, arr.shape, shape))
    b = library.product()
    out = {"length": np.zeros((h, w)), "prev_xy": np.zeros((h, w, 2)), "multiplier": np.zeros((h, w), dtype=np.uint8)}
    t = abi.Temporal(max_history=int(max_history), reserved0=0, depth_tolerance=depth_tolerance, normal_min=normal_min)
    ms = C.c_double(0.0)
    rc = b.temporal_probe(w, h, C.byref(cam), None if prev_cam is None else C.byref(prev_cam), f["normal"].ctypes.data, f["depth"].ctypes.data,
                          f["alpha"].ctypes.data, *[_ptr(x) for x in prev], C.byref(t), C.byref(a), *[_ptr(out[name]) for name in PROBE_OUTPUTS],
                          C.byref(ms))
    check(rc, b, "rttnw_temporal_probe")
    if want_ms:
        out["ms"] = ms.value
    return out


def orbit_cameras(cam, frames, step_degrees):
    """The cameras of an orbit of `frames` frames that ENDS at `cam`: frame k's lookfrom is `cam`'s, turned about the axis through lookat along
    view_up by (k - (frames - 1)) * step_degrees degrees (Rodrigues' formula); everything else is `cam`'s."""
    if int(frames) < 1:
        raise ValueError("orbit_cameras: at least one frame, got %r" % (frames,))
    at, up = np.array(cam.lookat[:], dtype=np.float64), np.array(cam.view_up[:], dtype=np.float64)
    axis = up / np.sqrt(np.dot(up, up))
    arm = np.array(cam.lookfrom[:], dtype=np.float64) - at
    cams = []
    for k in range(int(frames)):
        c = type(cam).from_buffer_copy(cam)
        if k != frames - 1:                      # the last frame is `cam`, bit for bit
            a = np.deg2rad((k - (frames - 1)) * step_degrees)
            turned = arm * np.cos(a) + np.cross(axis, arm) * np.sin(a) + axis * (np.dot(axis, arm) * (1.0 - np.cos(a)))
            for i in range(3):
                c.lookfrom[i] = at[i] + turned[i]
        cams.append(c)
    return cams


_spatial_denoise = denoise   # (render_sequence has a parameter of that name)


def render_sequence(scene, cams, params, temporal=True, denoise=False, iterations=5, max_history=0, depth_tolerance=0.0, normal_min=0.0,
                    on_frame=None, variance=False, clamp=None):
    """One frame per camera of `cams`: frame k is `render_host` with `sample_begin = params.sample_begin + k * params.spp` (so the frames are
    independent estimates), its `render_features` of min(spp, 16) samples, and — with `temporal` — `temporal_accumulate` over the previous
    frame's result.  With `denoise` the image shown is `rttnw_denoise` of the accumulated one; the history stays unfiltered.  Returns a list of
    dicts: "linear" and "rgba8" (the image to show), "raw" (the frame alone), "length" (None without `temporal`), "accumulated" (the
    `temporal_accumulate` result, None without `temporal`), "features", "cam", "stats" (the render's Stats).  `on_frame(k, frame)` is called
    as each frame is done.  With `variance` (which needs `temporal`) the frame goes through `temporal_variance` instead — accumulate, estimate,
    filter, the three stages of SVGF — and `rttnw_denoise` receives its "variance" for the colour stop; "accumulated" then carries "moment2"
    and "variance".  `clamp` (a number, which needs `variance`): the frames go through `temporal_clamp` with that gamma instead — the history is
    clipped to each frame's neighbourhood statistics before the blend — and "accumulated" carries "mean", "sd" and "clipped" as well; None, the
    default, leaves the frames as they are."""
    if variance and not temporal:
        raise ValueError("render_sequence: variance needs temporal: the variance is estimated from the accumulated history")
    if clamp is not None and not variance:
        raise ValueError("render_sequence: clamp needs variance: the clip stands in front of temporal_variance's blend")
    if clamp is not None and not float(clamp) >= 0.0:
        raise ValueError("render_sequence: clamp is the gamma of temporal_clamp, at least 0 (0: the default, 1.0), got %r" % (clamp,))
    frames, history = [], None
    for k, cam in enumerate(cams):
        p = copy.copy(params)
        p.sample_begin = params.sample_begin + k * params.spp
        raw, rgba, st = render_host(scene, cam, p)
        pf = copy.copy(p)
        pf.spp = min(p.spp, 16)
        features = render_features(scene, cam, pf)
        lin = raw
        if temporal:
            accumulate = temporal_variance if variance else temporal_accumulate
            if clamp is not None:
                accumulate = functools.partial(temporal_clamp, gamma=float(clamp))
            history = accumulate(raw, features, cam, history=history, max_history=max_history, depth_tolerance=depth_tolerance, normal_min=normal_min)
            lin, rgba = history["linear"], history["rgba8"]
        if denoise:
            lin, rgba, _ = _spatial_denoise(lin, features, None, iterations=iterations, variance=history["variance"] if variance else None)
        frame = {"linear": lin, "rgba8": rgba, "raw": raw, "length": history["length"] if temporal else None,
                 "accumulated": history if temporal else None, "features": features, "cam": cam, "stats": st}
        frames.append(frame)
        if on_frame is not None:
            on_frame(k, frame)
    return frames


SVGF_ARRAYS = {"linear_rgb": 3, "rgba8": 4, "accumulated_rgb": 3, "variance_rgb": 3, "filtered_variance_rgb": 3, "length": 0, "prev_xy": 2,
               "moment1_rgb": 3, "moment2_rgb": 3, "history_rgb": 3, "raw_rgb": 3, "albedo": 3, "normal": 3, "depth": 0, "alpha": 0}
HALVES_ARRAYS = ("acc_a", "acc_b", "filtered_a", "filtered_b", "fit")    # rttnw_svgf_halves' outputs, in its order
REGRESS_VARIANCE = ("temporal", "pair")                                  # rttnw_svgf_set_regress' variance_source 0, 1
SPATIAL_STAGES = ("atrous", "nlm", "regress")


class SvgfSequence:
    """An `rttnw_svgf` handle: a sequence's history on the device, and one call per frame — `frame` renders it, `push` takes a frame the caller
    rendered — that runs accumulate, estimate, filter and feed back without the host between them (include/rttnw_hip.h states the contract).
    `feedback` j: the colour history is the filter's result after j passes (0: the unfiltered accumulation, `render_sequence`'s); `demodulate`:
    everything the history holds is colour / albedo.  The other parameters are `temporal_variance`'s and `denoise`'s, a 0 their default.  Each
    call returns a dict of the outputs named in `want` (default: all of `SVGF_ARRAYS`), "image_ms" and "cam"; `frame` adds "stats".  A context
    manager: the handle is destroyed on exit."""

    def __init__(self, width, height, feedback=0, demodulate=False, feature_spp=0, iterations=5, sigma_luminance=0.0, sigma_normal=0.0, sigma_depth=0.0,
                 max_history=0, depth_tolerance=0.0, normal_min=0.0, min_temporal=0, radius=0, variance_sigma_normal=0.0, variance_sigma_depth=0.0):
        who = "SvgfSequence"
        if int(width) < 1 or int(height) < 1:
            raise ValueError("%s: width and height must be at least 1, got %r x %r" % (who, width, height))
        if not 0 <= int(iterations) <= 8:
            raise ValueError("%s: iterations must be 0 .. 8, got %r" % (who, iterations))
        if not 0 <= int(feedback) <= int(iterations):
            raise ValueError("%s: feedback must be 0 .. iterations (%d), got %r" % (who, iterations, feedback))
        self.width, self.height = int(width), int(height)
        self.params = abi.Svgf(feedback_iterations=int(feedback), demodulate=1 if demodulate else 0, feature_spp=int(feature_spp), reserved0=0,
                               t=abi.Temporal(max_history=int(max_history), reserved0=0, depth_tolerance=depth_tolerance, normal_min=normal_min),
                               v=abi.Variance(min_temporal=int(min_temporal), radius=int(radius), sigma_normal=variance_sigma_normal,
                                              sigma_depth=variance_sigma_depth, reserved0=0, reserved1=0),
                               d=_denoise_params(int(iterations), sigma_luminance, sigma_normal, sigma_depth))
        self._b = library.product()
        self.handle = C.c_void_p()
        check(self._b.svgf_create(self.width, self.height, C.byref(self.params), C.byref(self.handle)), self._b, "rttnw_svgf_create")

    def close(self):
        if self.handle:
            self._b.svgf_destroy(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        """Drop the history: the next call is a first frame."""
        check(self._b.svgf_reset(self.handle), self._b, "rttnw_svgf_reset")

    def set_clamp(self, gamma=0.0, radius=0, sigma_normal=0.0, sigma_depth=0.0):
        """`rttnw_svgf_set_clamp`: from the next call on the reprojected history — the moments' and, with feedback, the colour's — is clipped to the
        frame's neighbourhood statistics as `temporal_clamp` clips it (a 0: its default; a gamma of inf never clips).  The history is kept."""
        k = _clamp_params("SvgfSequence.set_clamp", gamma, radius, sigma_normal, sigma_depth)
        check(self._b.svgf_set_clamp(self.handle, C.byref(k)), self._b, "rttnw_svgf_set_clamp")

    def clear_clamp(self):
        """Clipping off again, from the next call on: the default."""
        check(self._b.svgf_set_clamp(self.handle, None), self._b, "rttnw_svgf_set_clamp")

    def clipped(self):
        """`rttnw_svgf_clipped`: HxW u8 of the last frame call — bits 0 - 2 the clipped channels of the first moment, bits 4 - 6 those of the
        fed-back colour history; all 0 before any call and after a call without a clamp."""
        out = np.zeros((self.height, self.width), dtype=np.uint8)
        check(self._b.svgf_clipped(self.handle, out.ctypes.data), self._b, "rttnw_svgf_clipped")
        return out

    def set_sampling(self, boost=0, fill=0.0):
        """`rttnw_svgf_set_sampling`: from the next `frame` call on, pixels whose reprojected history is thin are traced with up to `boost` times
        the frame's samples, as `temporal_probe` rules (a 0: its default, 8 and 8.0).  The history is kept.  Such a call may consume sample
        indices up to sample_begin + boost * spp: advance `sample_begin` by that much a frame.  Returns the boost in force."""
        a = _sampling_params("SvgfSequence.set_sampling", boost, fill)
        check(self._b.svgf_set_sampling(self.handle, C.byref(a)), self._b, "rttnw_svgf_set_sampling")
        return a.boost or 8

    def clear_sampling(self):
        """Sampling off again, from the next call on: the default."""
        check(self._b.svgf_set_sampling(self.handle, None), self._b, "rttnw_svgf_set_sampling")

    def samples(self):
        """`rttnw_svgf_samples`: (HxW u32, the samples each pixel of the last `frame` call was given; HxW f64, the reprojected history length the
        choice was made on).  Before any `frame` call both are 0; after one without sampling the first is that call's spp, the second 0."""
        spp, length = np.zeros((self.height, self.width), dtype=np.uint32), np.zeros((self.height, self.width))
        check(self._b.svgf_samples(self.handle, spp.ctypes.data, length.ctypes.data), self._b, "rttnw_svgf_samples")
        return spp, length

    def set_regress(self, mask=7, variance="temporal", ridge=0.0, search_radius=0, patch_radius=0, k=0.0):
        """`rttnw_svgf_set_regress`: from the next call on the spatial stage is `denoise_regress` over two half histories the handle accumulates
        beside the moments — with `mask` 0, `denoise_nlm`.  `variance`: "temporal" hands the filter the handle's temporal estimate (doubled: a half
        holds half the samples), "pair" leaves it its own pair variance.  The other parameters are `denoise_regress`'s, a 0 their default.  The
        history is dropped.  The stage is exclusive with feedback, a clamp and sampling; frames go in through `push_halves` or `frame` (an even spp)."""
        who = "SvgfSequence.set_regress"
        if variance not in REGRESS_VARIANCE:
            raise ValueError("%s: variance is one of %s, got %r" % (who, ", ".join(REGRESS_VARIANCE), variance))
        if not 0 <= int(mask) <= 7:
            raise ValueError("%s: mask must be 0 .. 7 (bits: 1 albedo, 2 normal, 4 depth), got %r" % (who, mask))
        if not ridge >= 0.0:
            raise ValueError("%s: ridge must be at least 0 (0: the library default), got %r" % (who, ridge))
        g = abi.Regress(search_radius=search_radius, patch_radius=patch_radius, k=k, ridge=ridge, features=int(mask), demodulate=0, reserved0=0, reserved1=0)
        check(self._b.svgf_set_regress(self.handle, C.byref(g), REGRESS_VARIANCE.index(variance)), self._b, "rttnw_svgf_set_regress")

    def clear_regress(self):
        """The à-trous filter as the spatial stage again: the default.  The history is dropped if the stage was set."""
        check(self._b.svgf_set_regress(self.handle, None, 0), self._b, "rttnw_svgf_set_regress")

    def halves(self, want=HALVES_ARRAYS):
        """`rttnw_svgf_halves`: a dict of the last frame call's "acc_a", "acc_b" (the accumulated halves), "filtered_a", "filtered_b" (the two fitted
        halves), HxWx3 each, and "fit" (HxW: how many of the two directions used the first-order value), in the filter's units; `want` names those
        to copy out.  All 0 before any call with the stage."""
        for name in want:
            if name not in HALVES_ARRAYS:
                raise ValueError("SvgfSequence.halves: no output named %r (there are %s)" % (name, ", ".join(HALVES_ARRAYS)))
        out = {name: np.zeros((self.height, self.width) if name == "fit" else (self.height, self.width, 3)) for name in want}
        check(self._b.svgf_halves(self.handle, *[_ptr(out.get(name)) for name in HALVES_ARRAYS]), self._b, "rttnw_svgf_halves")
        return out

    def push_halves(self, half_a, half_b, features, cam, want=None, no_outputs=False):
        """`rttnw_svgf_push_halves`: `push` on a handle with `set_regress` — the frame as the two halves `render_halves` returns."""
        a_, b_ = np.ascontiguousarray(half_a, dtype=np.float64), np.ascontiguousarray(half_b, dtype=np.float64)
        for arr in (a_, b_):
            if arr.shape != (self.height, self.width, 3):
                raise ValueError("SvgfSequence.push_halves: a half is %dx%dx3, got %s" % (self.height, self.width, arr.shape))
        f = _feature_arrays(features, self.height, self.width)
        arrays, out, ms = self._outputs(() if no_outputs else want)
        rc = self._b.svgf_push_halves(self.handle, C.byref(cam), a_.ctypes.data, b_.ctypes.data, f["albedo"].ctypes.data, f["normal"].ctypes.data,
                                      f["depth"].ctypes.data, f["alpha"].ctypes.data, None if no_outputs else C.byref(out))
        check(rc, self._b, "rttnw_svgf_push_halves")
        arrays["image_ms"], arrays["cam"] = ms.value, cam
        return arrays

    def _outputs(self, want):
        """(dict of zeroed arrays, the rttnw_svgf_out over them, the image_ms cell); `want` None: everything, () : nothing (no struct at all)."""
        names = tuple(SVGF_ARRAYS) if want is None else tuple(want)
        for name in names:
            if name not in SVGF_ARRAYS:
                raise ValueError("SvgfSequence: no output named %r (there are %s)" % (name, ", ".join(SVGF_ARRAYS)))
        h, w = self.height, self.width
        arrays = {name: np.zeros((h, w, SVGF_ARRAYS[name]) if SVGF_ARRAYS[name] else (h, w), dtype=np.uint8 if name == "rgba8" else np.float64)
                  for name in names}
        ms = C.c_double(0.0)
        out = abi.SvgfOut(image_ms=C.addressof(ms), **{name: a.ctypes.data for name, a in arrays.items()})
        return arrays, out, ms

    def push(self, linear, features, cam, want=None, no_outputs=False):
        """`rttnw_svgf_push`: a frame the caller rendered (`linear` HxWx3, `features` as `render_features` returns them).  `no_outputs`: the
        call is made with a NULL `out` and only advances the state."""
        lin = np.ascontiguousarray(linear, dtype=np.float64)
        if lin.shape != (self.height, self.width, 3):
            raise ValueError("SvgfSequence.push: the frame is %dx%dx3, got %s" % (self.height, self.width, lin.shape))
        f = _feature_arrays(features, self.height, self.width)
        arrays, out, ms = self._outputs(() if no_outputs else want)
        rc = self._b.svgf_push(self.handle, C.byref(cam), lin.ctypes.data, f["albedo"].ctypes.data, f["normal"].ctypes.data, f["depth"].ctypes.data,
                               f["alpha"].ctypes.data, None if no_outputs else C.byref(out))
        check(rc, self._b, "rttnw_svgf_push")
        arrays["image_ms"], arrays["cam"] = ms.value, cam
        return arrays

    def frame(self, scene, cam, params, want=None, no_outputs=False):
        """`rttnw_svgf_frame`: the frame rendered by the call itself, `rttnw_render`'s trace of `params` and the feature pass beside it."""
        arrays, out, ms = self._outputs(() if no_outputs else want)
        st = Stats()
        rc = self._b.svgf_frame(self.handle, scene.handle, C.byref(cam), C.byref(params), None if no_outputs else C.byref(out), C.byref(st))
        check(rc, self._b, "rttnw_svgf_frame")
        arrays["image_ms"], arrays["cam"], arrays["stats"] = ms.value, cam, st
        return arrays


def render_sequence_device(scene, cams, params, feedback=0, demodulate=False, iterations=5, max_history=0, depth_tolerance=0.0, normal_min=0.0,
                           on_frame=None, want=("linear_rgb", "rgba8", "raw_rgb", "length", "accumulated_rgb", "moment2_rgb", "variance_rgb", "prev_xy",
                                                "albedo", "normal", "depth", "alpha"), clamp=None, sampling=None, want_spp=False, spatial="atrous",
                           regress_variance="temporal", want_halves=False):
    """`render_sequence(..., variance=True, denoise=True)` on the device: one `SvgfSequence`, one `frame` call per camera, frame k at
    `sample_begin = params.sample_begin + k * params.spp`.  With `feedback` 0 and without `demodulate` the images are that function's, bit for
    bit.  Returns the same list of dicts — "linear", "rgba8", "raw", "length", "accumulated" ("linear", "rgba8" absent, "moment2", "variance",
    "length", "prev_xy"), "features", "cam", "stats" — and "image_ms", the device time behind the trace and the feature pass.  An entry of a
    frame is None where `want` leaves its output out.  `clamp` (a number): the handle clips its history with that gamma (`SvgfSequence.set_clamp`)
    and each frame carries "clipped", the call's map; None, the default, leaves the frames as they are.  `sampling` (a boost, or a pair
    (boost, fill); a 0: the default, 8 and 8.0): the handle gives pixels with a thin history up to boost times the frame's samples
    (`SvgfSequence.set_sampling`), and frame k starts at `sample_begin + k * boost * spp`; with `want_spp` each frame carries "spp" (HxW u32, the
    samples each pixel got) and "probe_length" (the reprojected history length behind the choice).  `spatial`: "atrous" (the default) filters with
    `rttnw_denoise`; "regress" and "nlm" make `denoise_regress` (every feature) or `denoise_nlm` the spatial stage over two accumulated halves
    (`SvgfSequence.set_regress`; an even spp; no feedback, clamp or sampling beside it), `regress_variance` ("temporal" or "pair") choosing the
    variances its weights read; with `want_halves` each frame carries "halves", what `SvgfSequence.halves` returns."""
    if spatial not in SPATIAL_STAGES:
        raise ValueError("render_sequence_device: spatial is one of %s, got %r" % (", ".join(SPATIAL_STAGES), spatial))
    if regress_variance not in REGRESS_VARIANCE:
        raise ValueError("render_sequence_device: regress_variance is one of %s, got %r" % (", ".join(REGRESS_VARIANCE), regress_variance))
    if spatial != "atrous":
        if feedback or clamp is not None or sampling is not None:
            raise ValueError("render_sequence_device: spatial=%r does not combine with feedback, clamp or sampling" % (spatial,))
        if params.spp < 2 or params.spp % 2:
            raise ValueError("render_sequence_device: spatial=%r traces two halves: spp must be even and at least 2, got %d" % (spatial, params.spp))
    if clamp is not None and not float(clamp) >= 0.0:
        raise ValueError("render_sequence_device: clamp is the gamma of temporal_clamp, at least 0 (0: the default, 1.0), got %r" % (clamp,))
    if sampling is not None:
        sampling = tuple(sampling) if isinstance(sampling, (tuple, list)) else (sampling, 0.0)
        if len(sampling) != 2:
            raise ValueError("render_sequence_device: sampling is a boost or a pair (boost, fill), got %r" % (sampling,))
        _sampling_params("render_sequence_device", *sampling)
    stride = 1
    frames = []
    with SvgfSequence(params.width, params.height, feedback=feedback, demodulate=demodulate, iterations=iterations, max_history=max_history,
                      depth_tolerance=depth_tolerance, normal_min=normal_min) as seq:
        if clamp is not None:
            seq.set_clamp(gamma=float(clamp))
        if sampling is not None:
            stride = seq.set_sampling(boost=sampling[0], fill=sampling[1])
        if spatial != "atrous":
            seq.set_regress(mask=7 if spatial == "regress" else 0, variance=regress_variance)
        for k, cam in enumerate(cams):
            p = copy.copy(params)
            p.sample_begin = params.sample_begin + k * stride * params.spp
            got = seq.frame(scene, cam, p, want=want)
            features = {name: got.get(name) for name in ("albedo", "normal", "depth", "alpha")}
            accumulated = {"linear": got.get("accumulated_rgb"), "moment2": got.get("moment2_rgb"), "variance": got.get("variance_rgb"),
                           "length": got.get("length"), "prev_xy": got.get("prev_xy"), "features": features, "cam": cam}
            frame = {"linear": got.get("linear_rgb"), "rgba8": got.get("rgba8"), "raw": got.get("raw_rgb"), "length": got.get("length"),
                     "accumulated": accumulated, "features": features, "cam": cam, "stats": got["stats"], "image_ms": got["image_ms"]}
            if clamp is not None:
                frame["clipped"] = seq.clipped()
            if want_spp:
                frame["spp"], frame["probe_length"] = seq.samples()
            if want_halves:
                frame["halves"] = seq.halves()
            frames.append(frame)
            if on_frame is not None:
                on_frame(k, frame)
    return frames


def lattice_mask(width, height, level):
    """The lattice of a preview as a mask (HxW u8): 1 where x % 2^level == 0 and y % 2^level == 0, row 0 at the top."""
    if not 0 <= int(level) <= 6:
        raise ValueError("lattice_mask: level must be 0 .. 6, got %r" % (level,))
    m = np.zeros((int(height), int(width)), dtype=np.uint8)
    m[:: 1 << int(level), :: 1 << int(level)] = 1
    return m


def reconstruct(linear, valid, features, stderr=None, iterations=5, sigma_luminance=0.0, sigma_normal=0.0, sigma_depth=0.0, want_ms=False,
                variance=None):
    """`rttnw_reconstruct`: `denoise` over an image of which only the pixels with a nonzero byte in `valid` (HxW) hold a value — the taps that
    hold nothing are dropped, the pixels that hold nothing are filled from those that do.  `stderr` (HxWx3) is squared into the variance of the
    pixel means; `variance` (HxWx3, in place of `stderr`) is that variance as it stands, so that an infinite, NaN or zero one arrives exactly.
    `linear`, `stderr` and `variance` are never read where `valid` is 0.
    Returns (linear HxWx3 f64, rgba8 HxWx4 u8 with alpha 0 where nothing could be filled, variance HxWx3 f64 or None, valid HxW u8) — and the
    device time in ms after them with `want_ms`."""
    b = library.product()
    lin = np.ascontiguousarray(linear, dtype=np.float64)
    h, w = lin.shape[:2]
    ok = np.ascontiguousarray(np.asarray(valid) != 0, dtype=np.uint8)
    if stderr is not None and variance is not None:
        raise ValueError("reconstruct: stderr or variance, not both")
    var = None if stderr is None else np.ascontiguousarray(np.square(np.asarray(stderr, dtype=np.float64)))
    if variance is not None:
        var = np.ascontiguousarray(variance, dtype=np.float64)
    assert lin.shape == (h, w, 3) and ok.shape == (h, w)
    f = _feature_arrays(features, h, w)
    assert var is None or var.shape == (h, w, 3)
    out = np.zeros((h, w, 3))
    rgba = np.zeros((h, w, 4), dtype=np.uint8)
    out_var = None if var is None else np.zeros((h, w, 3))
    out_ok = np.zeros((h, w), dtype=np.uint8)
    d = _denoise_params(iterations, sigma_luminance, sigma_normal, sigma_depth)
    ms = C.c_double(0.0)
    rc = b.reconstruct(w, h, lin.ctypes.data, _ptr(var), ok.ctypes.data, f["albedo"].ctypes.data, f["normal"].ctypes.data, f["depth"].ctypes.data,
                       f["alpha"].ctypes.data, C.byref(d), out.ctypes.data, rgba.ctypes.data, _ptr(out_var), out_ok.ctypes.data, C.byref(ms))
    check(rc, b, "rttnw_reconstruct")
    return (out, rgba, out_var, out_ok, ms.value) if want_ms else (out, rgba, out_var, out_ok)


def render_preview(scene, cam, params, level, pass_spp=64, rel_error=0.02, abs_error=0.0, iterations=5, feature_spp=0, sigma_luminance=0.0,
                   sigma_normal=0.0, sigma_depth=0.0, want_state=True):
    """`rttnw_render_preview`: the adaptive render of the lattice x % 2^level == 0, y % 2^level == 0 (1 pixel in 4^level), the features of the
    whole frame (`feature_spp` samples, 0 = pass_spp) and `reconstruct` over the two, on the device.  The same `spp_chunk` default as
    `render_adaptive`.  Returns a dict: "linear" HxWx3 f64 and "rgba8" HxWx4 u8 (the reconstructed image), "valid" HxW u8, "spp" HxW u32 (0 off
    the lattice), "raw_linear" and "raw_stderr" HxWx3 f64 (the lattice's own values), "state" (the frame-sized adaptive state with zero records
    off the lattice — `render_adaptive_region(..., 0, 0, W, H, state=...)` completes it — or None) and "stats"."""
    b = library.product()
    p = _pass_params(params, pass_spp)
    h, w = p.height, p.width
    out = {"linear": np.zeros((h, w, 3)), "rgba8": np.zeros((h, w, 4), dtype=np.uint8), "valid": np.zeros((h, w), dtype=np.uint8),
           "spp": np.zeros((h, w), dtype=np.uint32), "raw_linear": np.zeros((h, w, 3)), "raw_stderr": np.zeros((h, w, 3))}
    _, state = _state_arrays(b, "render_preview", p, None, want_state)
    st = Stats()
    a = abi.Adaptive(pass_spp=pass_spp, reserved0=0, rel_error=rel_error, abs_error=abs_error)
    v = abi.Preview(level=level, feature_spp=feature_spp, denoise=_denoise_params(iterations, sigma_luminance, sigma_normal, sigma_depth))
    rc = b.render_preview(scene.handle, C.byref(cam), C.byref(p), C.byref(a), C.byref(v), out["linear"].ctypes.data, out["rgba8"].ctypes.data,
                          out["valid"].ctypes.data, out["spp"].ctypes.data, out["raw_linear"].ctypes.data, out["raw_stderr"].ctypes.data,
                          _ptr(state), C.byref(st))
    check(rc, b, "rttnw_render_preview")
    out["state"] = state
    out["stats"] = st
    return out


def budget_select(linear, stderr, spp, cap, rel_error, abs_error, max_pixels, want_ms=False):
    """`rttnw_budget_select`: which pixels get the next adaptive pass when only `max_pixels` of them can — the candidates (no samples yet, or
    below `cap` and short of stderr <= abs_error + rel_error * mean in some channel) ranked by priority = max over r, g, b of stderr / tolerance,
    descending, then by row-major index.  `linear` and `stderr` (HxWx3) are never read where `spp` (HxW) is 0.  Returns (mask HxW u8, priority HxW
    f64 — 0 for a non-candidate, +inf for a pixel without samples —, the number selected) — and the device time in ms after them with `want_ms`."""
    b = library.product()
    n = np.ascontiguousarray(spp, dtype=np.uint32)
    h, w = n.shape
    lin = np.ascontiguousarray(linear, dtype=np.float64)
    se = np.ascontiguousarray(stderr, dtype=np.float64)
    assert lin.shape == (h, w, 3) and se.shape == (h, w, 3)
    mask = np.zeros((h, w), dtype=np.uint8)
    rho = np.zeros((h, w), dtype=np.float64)
    m, ms = C.c_uint64(0), C.c_double(0.0)
    rc = b.budget_select(w, h, lin.ctypes.data, se.ctypes.data, n.ctypes.data, cap, rel_error, abs_error, int(max_pixels), mask.ctypes.data,
                         rho.ctypes.data, C.byref(m), C.byref(ms))
    check(rc, b, "rttnw_budget_select")
    return (mask, rho, int(m.value), ms.value) if want_ms else (mask, rho, int(m.value))


def render_adaptive_budget(scene, cam, params, samples, round_pixels=0, state=None, pass_spp=64, rel_error=0.02, abs_error=0.0, want_state=True):
    """`rttnw_render_adaptive_budget`: the adaptive render under a budget — at most `samples` camera paths, spent in rounds of at most
    `round_pixels` pixels (0 = half the frame), each round giving one more pass of `pass_spp` samples to the pixels `budget_select` ranks
    worst under the tolerances and `params.spp` (the cap).  `state` is the frame-sized array an adaptive call returned (a pixel never sampled is a
    record of zeros); None stands for all zeros.  The same `spp_chunk` default as `render_adaptive`.  Returns (linear HxWx3 f64, rgba8 HxWx4 u8,
    spp_map HxW u32, stderr HxWx3 f64, Stats, state or None, rounds run); a pixel without samples is zero everywhere, alpha included."""
    b = library.product()
    p = _pass_params(params, pass_spp)
    lin, rgba, spp, se = _frame_outputs(p.height, p.width)
    st_in, st_out = _state_arrays(b, "render_adaptive_budget", p, state, want_state)
    st = Stats()
    a = abi.Adaptive(pass_spp=pass_spp, reserved0=0, rel_error=rel_error, abs_error=abs_error)
    bg = abi.Budget(samples=int(samples), round_pixels=int(round_pixels), reserved0=0)
    rc = b.render_adaptive_budget(scene.handle, C.byref(cam), C.byref(p), C.byref(a), C.byref(bg), _ptr(st_in), _ptr(st_out), lin.ctypes.data,
                                  rgba.ctypes.data, spp.ctypes.data, se.ctypes.data, C.byref(st))
    check(rc, b, "rttnw_render_adaptive_budget")
    return lin, rgba, spp, se, st, st_out, st.reserved >> 16


def render_adaptive_budget_denoised(scene, cam, params, samples, round_pixels=0, state=None, pass_spp=64, rel_error=0.02, abs_error=0.0, iterations=5,
                                    feature_spp=0, sigma_luminance=0.0, sigma_normal=0.0, sigma_depth=0.0, want_state=True):
    """`rttnw_render_adaptive_budget_denoised`: `render_adaptive_budget` whose rounds rank pixels by the noise of the FILTERED image — each round the
    frame goes through `reconstruct`'s passes on the device (features of `feature_spp` samples, 0 = pass_spp; a pixel may hold nothing yet) and
    `budget_select` runs on the filtered image and sqrt(filtered variance), a pixel whose own standard error is 0 set aside.  `state` as in
    `render_adaptive_budget`.  The same `spp_chunk` default as `render_adaptive`.  Returns a dict like `render_preview`'s: "linear" HxWx3 f64, "rgba8"
    HxWx4 u8 and "valid" HxW u8 (the filtered image), "stderr" HxWx3 f64 (sqrt of the filtered variance, +inf where nothing is valid), "spp" HxW u32,
    "raw_linear" and "raw_stderr" HxWx3 f64 (`render_adaptive_budget`'s values), "state" (or None), "rounds" (rounds that traced) and "stats"."""
    b = library.product()
    p = _pass_params(params, pass_spp)
    h, w = p.height, p.width
    out = {"linear": np.zeros((h, w, 3)), "rgba8": np.zeros((h, w, 4), dtype=np.uint8), "valid": np.zeros((h, w), dtype=np.uint8),
           "spp": np.zeros((h, w), dtype=np.uint32), "stderr": np.zeros((h, w, 3)), "raw_linear": np.zeros((h, w, 3)), "raw_stderr": np.zeros((h, w, 3))}
    st_in, st_out = _state_arrays(b, "render_adaptive_budget_denoised", p, state, want_state)
    st = Stats()
    a = abi.Adaptive(pass_spp=pass_spp, reserved0=0, rel_error=rel_error, abs_error=abs_error)
    bg = abi.Budget(samples=int(samples), round_pixels=int(round_pixels), reserved0=0)
    g = abi.Guided(feature_spp=feature_spp, reserved0=0, denoise=_denoise_params(iterations, sigma_luminance, sigma_normal, sigma_depth))
    rc = b.render_adaptive_budget_denoised(scene.handle, C.byref(cam), C.byref(p), C.byref(a), C.byref(bg), C.byref(g), _ptr(st_in), _ptr(st_out),
                                           out["linear"].ctypes.data, out["rgba8"].ctypes.data, out["valid"].ctypes.data, out["spp"].ctypes.data,
                                           out["stderr"].ctypes.data, out["raw_linear"].ctypes.data, out["raw_stderr"].ctypes.data, C.byref(st))
    check(rc, b, "rttnw_render_adaptive_budget_denoised")
    out["state"] = st_out
    out["rounds"] = st.reserved >> 16
    out["stats"] = st
    return out


def render_host_passes(scene, cam, params, passes, on_pass=None):
    """The same image as `render_host`, in `passes` passes over disjoint sample ranges (`rttnw_params.sample_begin`):
    after every pass the running mean is a complete, displayable estimate — progressive display and a natural
    checkpoint (persist the running sum and the next sample index) for long renders.  `on_pass(k, linear)` is called
    with the running mean after pass k.  Returns (linear HxWx3 f64, rgba8 HxWx4 u8, samples per pixel done)."""
    import copy
    total, done = None, 0
    base, spp = params.sample_begin, params.spp
    for k in range(passes):
        n = spp // passes + (1 if k < spp % passes else 0)
        if n == 0:
            continue
        p = copy.copy(params)
        p.spp, p.sample_begin = n, base + done
        lin, _, _ = render_host(scene, cam, p, want_stats=False)
        total = lin * n if total is None else total + lin * n
        done += n
        if on_pass is not None:
            on_pass(k, total / done)
    mean = total / max(done, 1)
    return mean, quantise_rgba8(mean), done


def quantise_rgba8(linear):
    """main.rs:219-225 on a linear image: sqrt, clamp to 0.999, * 256, `as u8`; alpha 255."""
    x = np.sqrt(np.maximum(linear, 0.0))
    x = np.minimum(x, 0.999) * 256.0
    rgba = np.full(linear.shape[:2] + (4,), 255, dtype=np.uint8)
    rgba[..., :3] = np.nan_to_num(x, nan=0.0).astype(np.uint8)
    return rgba


def _torch_dtype(precision):
    import torch
    return torch.float32 if precision == abi.F32 else torch.float64


class DeviceRenderer:
    """Device-resident render of this rank's tiles (+ gather over torch.distributed for world > 1).

    Buffers are torch tensors on the current device; kernels are launched on torch's current stream.
    """

    def __init__(self, scene, cam, params, group=None):
        import torch
        self.torch = torch
        self.b = library.product()
        self.scene, self.cam, self.params = scene, cam, params
        self.world = params.tile_world
        self.rank = params.tile_rank
        self.group = group
        self.lay = tiles.layout(params.width, params.height, self.world)
        dt = _torch_dtype(params.precision)
        dev = torch.device("cuda", torch.cuda.current_device())
        self.packed = torch.zeros((self.lay["pixels_per_rank"], 4), dtype=dt, device=dev)
        root = self.rank == 0
        # force_gather: run the collective with a single rank too (launch-plumbing check on a 1-GPU box)
        self.force_gather = bool(group is None and self.world == 1 and __import__("os").environ.get("RTTNW_BENCH_FORCE_DIST") == "1")
        self.gathered = (torch.zeros((self.world, self.lay["pixels_per_rank"], 4), dtype=dt, device=dev)
                         if (root and (self.world > 1 or self.force_gather)) else None)
        self.linear = torch.zeros((params.height, params.width, 3), dtype=dt, device=dev) if root else None
        self.rgba8 = torch.zeros((params.height, params.width, 4), dtype=torch.uint8, device=dev) if root else None

    def trace(self, stats=None):
        """Launch the trace + resolve kernels for this rank's tiles (asynchronous)."""
        stream = self.torch.cuda.current_stream().cuda_stream
        rc = self.b.render_tiles_device(self.scene.handle, C.byref(self.cam), C.byref(self.params),
                                        self.packed.data_ptr(), stream, C.byref(stats) if stats is not None else None)
        check(rc, self.b, "rttnw_render_tiles_device")

    def collect(self):
        """Gather every rank's packed tiles on rank 0 (RCCL over xGMI) and scatter them into the framebuffer."""
        src = self.packed
        if self.world > 1 or self.force_gather:
            import torch.distributed as dist
            if dist.get_backend(self.group) == "gloo":
                # rehearsal of an N-rank run on ONE device (bench.py RTTNW_BENCH_ONE_DEVICE=1; RCCL refuses two ranks on a device):
                # gloo gathers host tensors only, so the packed tiles go through the host
                host = self.packed.cpu()
                hlist = [self.torch.empty_like(host) for _ in range(self.world)] if self.rank == 0 else None
                dist.gather(host, hlist, dst=0, group=self.group)
                if self.rank == 0:
                    self.gathered.copy_(self.torch.stack(hlist))
            else:
                glist = list(self.gathered.unbind(0)) if self.rank == 0 else None
                dist.gather(self.packed, glist, dst=0, group=self.group)   # RCCL: grouped send/recv into rank 0
            src = self.gathered
        if self.rank == 0:
            p = self.params
            stream = self.torch.cuda.current_stream().cuda_stream
            rc = self.b.untile_device(p.width, p.height, self.world, p.precision, src.data_ptr(),
                                      self.linear.data_ptr(), self.rgba8.data_ptr(), stream)
            check(rc, self.b, "rttnw_untile_device")

    def step(self):
        self.trace()
        self.collect()
