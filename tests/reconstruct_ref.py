"""TEST INFRASTRUCTURE for rttnw_reconstruct: a tap-ordered numpy restatement of the filter over a partly valid image, written from the
contract in include/rttnw_hip.h (not from rttnw_amd/csrc/reconstruct.hpp), and the loader of the host build of that header
(tests/reconstruct_host).  numpy's element-wise double arithmetic is IEEE and fuses nothing, so the three — device, host build, this file —
must agree bit for bit, for every validity pattern.  An invalid pixel's colour and variance are replaced by 0 before any arithmetic here and
every use of a tap is guarded by its flag, so a NaN there can only reach the output through a mistake in the flags."""
import ctypes as C
import os
import subprocess

import numpy as np

from denoise_ref import ALBEDO_EPS, B3, DEFAULTS, ROOT, TINY, _lum, _shift, quantise


def host():
    """rh_reconstruct of tests/reconstruct_host, wrapped: (colour, variance or None, valid, features, iterations, sigmas) ->
    (colour, rgba8, variance or None, valid)."""
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "reconstruct_host"), "-s"], check=True)
    lib = C.CDLL(os.path.join(ROOT, "tests", "reconstruct_host", "libreconstruct_host.so"))
    lib.rh_reconstruct.argtypes = [C.c_uint32, C.c_uint32] + [C.c_void_p] * 7 + [C.c_uint32, C.c_double, C.c_double, C.c_double] + [C.c_void_p] * 4
    lib.rh_reconstruct.restype = C.c_int

    def run(colour, variance, valid, f, iterations, sigma_luminance=0.0, sigma_normal=0.0, sigma_depth=0.0):
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (colour, f["albedo"], f["normal"], f["depth"], f["alpha"])]
        var = None if variance is None else np.ascontiguousarray(variance, dtype=np.float64)
        ok = np.ascontiguousarray(np.asarray(valid) != 0, dtype=np.uint8)
        h, w = arrs[0].shape[:2]
        assert arrs[0].shape == (h, w, 3) and arrs[1].shape == (h, w, 3) and arrs[2].shape == (h, w, 3) and arrs[3].shape == (h, w)
        assert arrs[4].shape == (h, w) and ok.shape == (h, w) and (var is None or var.shape == (h, w, 3))
        out, rgba, out_ok = np.zeros((h, w, 3)), np.zeros((h, w, 4), dtype=np.uint8), np.zeros((h, w), dtype=np.uint8)
        out_var = None if var is None else np.zeros((h, w, 3))
        rc = lib.rh_reconstruct(w, h, arrs[0].ctypes.data, None if var is None else var.ctypes.data, ok.ctypes.data, arrs[1].ctypes.data,
                                arrs[2].ctypes.data, arrs[3].ctypes.data, arrs[4].ctypes.data, iterations, sigma_luminance, sigma_normal,
                                sigma_depth, out.ctypes.data, rgba.ctypes.data, None if out_var is None else out_var.ctypes.data, out_ok.ctypes.data)
        assert rc == 0
        return out, rgba, out_var, out_ok
    return run


def lattice(w, h, level):
    """The validity pattern of a preview: x % 2^level == 0 and y % 2^level == 0."""
    m = np.zeros((h, w), dtype=bool)
    m[:: 1 << level, :: 1 << level] = True
    return m


def _pass(c, v, H, normal, depth, alpha, stride, sl, squarings, sz):
    hit = alpha != 0.0
    own = hit & H                       # centres that run rttnw_denoise's operations
    fill = hit & ~H                     # centres that are filled
    lum = _lum(c)
    use_l = np.zeros_like(hit)
    scale = None
    fin = None
    if v is not None:
        fin = np.isfinite(v).all(axis=-1)
        use_l = own & fin
        lv = (0.2126 * 0.2126) * v[..., 0] + (0.7152 * 0.7152) * v[..., 1] + (0.0722 * 0.0722) * v[..., 2]
        s, sw = np.zeros_like(lum), np.zeros_like(lum)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                lv_q, inside = _shift(lv, dy, dx)
                ok = inside & _shift(hit, dy, dx, False)[0] & _shift(H, dy, dx, False)[0] & _shift(fin, dy, dx, False)[0]
                wt = float((2 - abs(dx)) * (2 - abs(dy)))
                with np.errstate(all="ignore"):
                    s = np.where(ok, s + wt * lv_q, s)
                sw = np.where(ok, sw + wt, sw)
        with np.errstate(all="ignore"):
            V = s / sw
            scale = sl * np.sqrt(np.where(V > 0.0, V, 0.0)) + TINY
    sum_w, sum_c = np.zeros_like(lum), np.zeros_like(c)
    sum_v = None if v is None else np.zeros_like(c)
    any_v = np.zeros_like(hit)
    az0 = np.abs(depth)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            oy, ox = dy * stride, dx * stride
            _, inside = _shift(lum, oy, ox)
            accepted = inside & _shift(hit, oy, ox, False)[0] & _shift(H, oy, ox, False)[0] & hit
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
                sum_w = np.where(accepted, sum_w + w, sum_w)
                sum_c = np.where(accepted[..., None], sum_c + w[..., None] * c_q, sum_c)
                if v is not None:
                    v_q = _shift(v, oy, ox)[0]
                    tv = accepted & (use_l | fill) & _shift(fin, oy, ox, False)[0]
                    sum_v = np.where(tv[..., None], sum_v + (w * w)[..., None] * v_q, sum_v)
                    any_v = any_v | tv
    got = hit & (sum_w > 0.0)
    with np.errstate(all="ignore"):
        out_c = np.where(got[..., None], sum_c / sum_w[..., None], c)
        out_v = None
        if v is not None:
            out_v = np.where((got & use_l)[..., None], sum_v / (sum_w * sum_w)[..., None], v)
            out_v = np.where((got & fill)[..., None], np.where(any_v[..., None], sum_v / (sum_w * sum_w)[..., None], np.inf), out_v)
    return out_c, out_v, H | (got & fill)


def reconstruct(colour, variance, valid, f, iterations, sigma_luminance=0.0, sigma_normal=0.0, sigma_depth=0.0):
    """The contract of rttnw_reconstruct restated: (colour, rgba8, variance or None, valid u8)."""
    H = np.asarray(valid) != 0
    colour = np.where(H[..., None], np.asarray(colour, dtype=np.float64), 0.0)          # never read where H is 0
    variance = None if variance is None else np.where(H[..., None], np.asarray(variance, dtype=np.float64), 0.0)
    albedo, alpha = f["albedo"], f["alpha"]
    if iterations == 0:
        c, v, mod = colour, variance, np.zeros_like(albedo, dtype=bool)
    else:
        sl = sigma_luminance or DEFAULTS["sigma_luminance"]
        sn = sigma_normal or DEFAULTS["sigma_normal"]
        sz = sigma_depth or DEFAULTS["sigma_depth"]
        squarings = 0
        while squarings < 10 and float(1 << squarings) < sn:
            squarings += 1
        mod = (alpha[..., None] != 0.0) & (albedo > ALBEDO_EPS)
        with np.errstate(all="ignore"):
            c = np.where(mod, colour / albedo, colour)
            v = None if variance is None else np.where(mod, variance / (albedo * albedo), variance)
        sky = ~H & (alpha == 0.0)                                                     # the background a miss returns
        c = np.where(sky[..., None], albedo, c)
        v = None if v is None else np.where(sky[..., None], 0.0, v)
        H = H | sky
        for i in range(iterations):
            c, v, H = _pass(c, v, H, f["normal"], f["depth"], alpha, 1 << i, sl, squarings, sz)
    with np.errstate(all="ignore"):
        out = np.where(H[..., None], np.where(mod, c * albedo, c), 0.0)
        out_v = None if v is None else np.where(H[..., None], np.where(mod, v * (albedo * albedo), v), np.inf)
    rgba = quantise(out)
    rgba[~H] = 0
    return out, rgba, out_v, H.astype(np.uint8)
