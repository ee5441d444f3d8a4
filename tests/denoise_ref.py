"""TEST INFRASTRUCTURE for rttnw_denoise: a tap-ordered numpy restatement of the filter, written from the contract in
include/rttnw_hip.h (not from rttnw_amd/csrc/denoise.hpp), and the loader of the host build of that header (tests/denoise_host).
numpy's element-wise double arithmetic is IEEE and fuses nothing, so the three — device, host build, this file — must agree bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALBEDO_EPS, TINY = 1e-3, 1e-12
DEFAULTS = {"sigma_luminance": 4.0, "sigma_normal": 64.0, "sigma_depth": 0.1}
B3 = (1, 4, 6, 4, 1)


def host():
    """dh_denoise of tests/denoise_host, wrapped: (colour, variance or None, features, iterations, sigmas) -> (colour, rgba8, variance)."""
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "denoise_host"), "-s"], check=True)
    lib = C.CDLL(os.path.join(ROOT, "tests", "denoise_host", "libdenoise_host.so"))
    lib.dh_denoise.argtypes = [C.c_uint32, C.c_uint32] + [C.c_void_p] * 6 + [C.c_uint32, C.c_double, C.c_double, C.c_double] + [C.c_void_p] * 3
    lib.dh_denoise.restype = C.c_int

    def run(colour, variance, f, iterations, sigma_luminance=0.0, sigma_normal=0.0, sigma_depth=0.0):
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (colour, f["albedo"], f["normal"], f["depth"], f["alpha"])]
        var = None if variance is None else np.ascontiguousarray(variance, dtype=np.float64)
        h, w = arrs[0].shape[:2]
        out, rgba = np.zeros((h, w, 3)), np.zeros((h, w, 4), dtype=np.uint8)
        out_var = None if var is None else np.zeros((h, w, 3))
        rc = lib.dh_denoise(w, h, arrs[0].ctypes.data, None if var is None else var.ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data,
                            arrs[3].ctypes.data, arrs[4].ctypes.data, iterations, sigma_luminance, sigma_normal, sigma_depth,
                            out.ctypes.data, rgba.ctypes.data, None if out_var is None else out_var.ctypes.data)
        assert rc == 0
        return out, rgba, out_var
    return run


def _shift(a, dy, dx, fill=0.0):
    """out[y, x] = a[y + dy, x + dx] where that lies inside the image (else `fill`), and the mask of where it does."""
    h, w = a.shape[:2]
    out = np.full_like(a, fill)
    inside = np.zeros((h, w), dtype=bool)
    y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        inside[y0:y1, x0:x1] = True
    return out, inside


def _lum(c):
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


def _pass(c, v, normal, depth, alpha, stride, sl, squarings, sz):
    hit = alpha != 0.0
    lum = _lum(c)
    use_l = np.zeros_like(hit)
    scale = None
    if v is not None:
        fin = np.isfinite(v).all(axis=-1)
        use_l = hit & fin
        lv = (0.2126 * 0.2126) * v[..., 0] + (0.7152 * 0.7152) * v[..., 1] + (0.0722 * 0.0722) * v[..., 2]
        s, sw = np.zeros_like(lum), np.zeros_like(lum)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                lv_q, inside = _shift(lv, dy, dx)
                ok = inside & _shift(hit, dy, dx, False)[0] & _shift(fin, dy, dx, False)[0]
                wt = float((2 - abs(dx)) * (2 - abs(dy)))
                with np.errstate(all="ignore"):
                    s = np.where(ok, s + wt * lv_q, s)
                sw = np.where(ok, sw + wt, sw)
        with np.errstate(all="ignore"):
            V = s / sw
            scale = sl * np.sqrt(np.where(V > 0.0, V, 0.0)) + TINY
    sum_w, sum_c = np.zeros_like(lum), np.zeros_like(c)
    sum_v = None if v is None else np.zeros_like(c)
    az0 = np.abs(depth)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            oy, ox = dy * stride, dx * stride
            _, inside = _shift(lum, oy, ox)
            hit_q = _shift(hit, oy, ox, False)[0]
            valid = inside & hit_q & hit
            h = float(B3[dx + 2] * B3[dy + 2]) / 256.0
            n_q = _shift(normal, oy, ox)[0]
            d = normal[..., 0] * n_q[..., 0] + normal[..., 1] * n_q[..., 1] + normal[..., 2] * n_q[..., 2]
            wn = np.where(d > 0.0, d, 0.0)
            for _ in range(squarings):
                wn = wn * wn
            z_q = _shift(depth, oy, ox)[0]
            with np.errstate(all="ignore"):
                qz = (depth - z_q) / ((sz * (az0 + np.abs(z_q))) * 0.5 + TINY)
                rz = 1.0 / (1.0 + qz * qz)
                wz = rz * rz
                wl = np.ones_like(lum)
                if v is not None:
                    ql = (lum - _shift(lum, oy, ox)[0]) / scale
                    wl = np.where(use_l, 1.0 / (1.0 + ql * ql), 1.0)
                w = ((h * wn) * wz) * wl
                c_q = _shift(c, oy, ox)[0]
                sum_w = np.where(valid, sum_w + w, sum_w)
                sum_c = np.where(valid[..., None], sum_c + w[..., None] * c_q, sum_c)
                if v is not None:
                    v_q = _shift(v, oy, ox)[0]
                    tv = valid & use_l & _shift(fin, oy, ox, False)[0]
                    sum_v = np.where(tv[..., None], sum_v + (w * w)[..., None] * v_q, sum_v)
    ok = hit & (sum_w > 0.0)
    with np.errstate(all="ignore"):
        out_c = np.where(ok[..., None], sum_c / sum_w[..., None], c)
        out_v = None if v is None else np.where((ok & use_l)[..., None], sum_v / (sum_w * sum_w)[..., None], v)
    return out_c, out_v


def quantise(linear):
    """main.rs:219-225: sqrt, clamp to [0, 0.999], * 256, `as u8` (NaN -> 0); alpha 255."""
    with np.errstate(all="ignore"):
        x = np.sqrt(linear)
    x = np.where(x < 0.0, 0.0, x)
    x = np.where(x > 0.999, 0.999, x) * 256.0
    x = np.where(np.isnan(x) | (x <= 0.0), 0.0, np.minimum(x, 255.0))
    rgba = np.full(linear.shape[:2] + (4,), 255, dtype=np.uint8)
    rgba[..., :3] = x.astype(np.uint8)
    return rgba


def denoise(colour, variance, f, iterations, sigma_luminance=0.0, sigma_normal=0.0, sigma_depth=0.0):
    """The contract of rttnw_denoise restated: (colour, rgba8, variance or None)."""
    colour = np.asarray(colour, dtype=np.float64)
    variance = None if variance is None else np.asarray(variance, dtype=np.float64)
    if iterations == 0:
        return colour.copy(), quantise(colour), None if variance is None else variance.copy()
    sl = sigma_luminance or DEFAULTS["sigma_luminance"]
    sn = sigma_normal or DEFAULTS["sigma_normal"]
    sz = sigma_depth or DEFAULTS["sigma_depth"]
    squarings = 0
    while squarings < 10 and float(1 << squarings) < sn:
        squarings += 1
    albedo, alpha = f["albedo"], f["alpha"]
    mod = (alpha[..., None] != 0.0) & (albedo > ALBEDO_EPS)
    with np.errstate(all="ignore"):
        c = np.where(mod, colour / albedo, colour)
        v = None if variance is None else np.where(mod, variance / (albedo * albedo), variance)
    for i in range(iterations):
        c, v = _pass(c, v, f["normal"], f["depth"], alpha, 1 << i, sl, squarings, sz)
    with np.errstate(all="ignore"):
        out = np.where(mod, c * albedo, c)
        out_v = None if v is None else np.where(mod, v * (albedo * albedo), v)
    return out, quantise(out), out_v


def random_inputs(rng, w, h, with_variance=True):
    """A frame that reaches every branch: flat and noisy normals, depth steps, alpha 0 / fractional / 1, albedo channels below the
    demodulation threshold, variances that are zero, huge, infinite and NaN."""
    base = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [0.6, 0.0, 0.8], [-1.0, 0.0, 0.0]])
    region = (np.add.outer(np.arange(h) // 9, np.arange(w) // 11)) % 4
    normal = base[region] + 0.05 * rng.standard_normal((h, w, 3))
    normal *= rng.choice([1.0, 1.0, 1.0, 0.7, 0.3], size=(h, w, 1))                # silhouettes: shorter than 1
    depth = 5.0 + 3.0 * region + 0.02 * np.add.outer(np.arange(h), np.arange(w)) + 0.01 * rng.random((h, w))
    alpha = rng.choice([1.0, 1.0, 1.0, 1.0, 0.75, 0.25, 0.0], size=(h, w))
    alpha[: h // 6, : w // 5] = 0.0                                                # a block of sky
    albedo = rng.random((h, w, 3)) * rng.choice([1.0, 1.0, 1.0, 5e-4, 0.0], size=(h, w, 3))
    colour = albedo * rng.exponential(1.0, size=(h, w, 3)) + (rng.random((h, w, 3)) < 0.02) * rng.exponential(30.0, size=(h, w, 3))
    f = {"albedo": albedo, "normal": normal, "depth": depth, "alpha": alpha}
    var = None
    if with_variance:
        var = (0.3 * colour) ** 2 * rng.exponential(1.0, size=(h, w, 3))
        kind = rng.random((h, w))
        var[kind < 0.03] = np.inf
        var[(kind >= 0.03) & (kind < 0.05)] = np.nan
        var[(kind >= 0.05) & (kind < 0.08)] = 0.0
    return colour, var, f
