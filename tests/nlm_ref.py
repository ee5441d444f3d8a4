"""TEST INFRASTRUCTURE for rttnw_denoise_nlm: a numpy restatement of the filter, written from the contract in include/rttnw_hip.h (not from
rttnw_amd/csrc/nlm.hpp), and the loader of the host build of that header (tests/nlm_host).  numpy's element-wise double arithmetic is IEEE and
fuses nothing, and every sum below adds its terms one at a time in the header's order, so the three — device, host build, this file — must
agree bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from denoise_ref import quantise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = {"search_radius": 7, "patch_radius": 3, "k": 0.7}
OUTPUTS = ("linear", "rgba8", "half_a", "half_b", "error")


def host():
    """nh_denoise_nlm of tests/nlm_host, wrapped: (half_a, half_b, var_a or None, var_b or None, r, f, k) -> dict of the five outputs."""
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "nlm_host"), "-s"], check=True)
    lib = C.CDLL(os.path.join(ROOT, "tests", "nlm_host", "libnlm_host.so"))
    lib.nh_denoise_nlm.argtypes = [C.c_uint32, C.c_uint32] + [C.c_void_p] * 4 + [C.c_uint32, C.c_uint32, C.c_double] + [C.c_void_p] * 5
    lib.nh_denoise_nlm.restype = C.c_int

    def run(half_a, half_b, var_a=None, var_b=None, search_radius=0, patch_radius=0, k=0.0):
        arrs = [None if x is None else np.ascontiguousarray(x, dtype=np.float64) for x in (half_a, half_b, var_a, var_b)]
        h, w = arrs[0].shape[:2]
        out = {"linear": np.zeros((h, w, 3)), "rgba8": np.zeros((h, w, 4), dtype=np.uint8), "half_a": np.zeros((h, w, 3)),
               "half_b": np.zeros((h, w, 3)), "error": np.zeros((h, w, 3))}
        rc = lib.nh_denoise_nlm(w, h, *[None if x is None else x.ctypes.data for x in arrs], search_radius, patch_radius, k,
                                *[out[name].ctypes.data for name in OUTPUTS])
        assert rc == 0
        return out
    return run


def _extend(a, n):
    """The image with n more pixels on every side, each the nearest pixel inside: a coordinate clamped to the image."""
    return np.pad(a, ((n, n), (n, n)) + ((0, 0),) * (a.ndim - 2), mode="edge")


def pair_variance(a, b):
    h, w = a.shape[:2]
    d = a - b
    pv = _extend((d * d) * 0.5, 1)
    s = np.zeros_like(a)
    for dy in range(3):
        for dx in range(3):
            s = s + pv[dy:dy + h, dx:dx + w]
    return s / 9.0


def _cross_filter(guide, var, src, r, f, k2):
    """`src` averaged with the weights found in `guide` (variance `var`).  One row of offsets (all ox of an oy) is evaluated at a time; the
    candidates are then accumulated one offset after the other, row-major."""
    h, w = guide.shape[:2]
    ph, pw = h + 2 * f, w + 2 * f                                   # the image and its patch halo: extended coordinates -f .. n + f
    ge, ve, se = _extend(guide, r + f), _extend(var, r + f), _extend(src, r)
    gx, vx = ge[r:r + ph, r:r + pw][None], ve[r:r + ph, r:r + pw][None]
    taps = float(3 * (2 * f + 1) ** 2)
    sum_w, sum_c = np.zeros((h, w)), np.zeros((h, w, 3))
    with np.errstate(all="ignore"):
        for oy in range(-r, r + 1):
            # [ox + r, y, x, channel]: the guide and its variance at q = x + (ox, oy)
            gq = sliding_window_view(ge[r + oy:r + oy + ph], pw, axis=1).transpose(1, 0, 3, 2)
            vq = sliding_window_view(ve[r + oy:r + oy + ph], pw, axis=1).transpose(1, 0, 3, 2)
            d = gx - gq
            dc = (d * d - (vx + np.where(vx < vq, vx, vq))) / (1e-10 + k2 * (vx + vq))
            delta = (dc[..., 0] + dc[..., 1]) + dc[..., 2]
            rows = np.zeros((2 * r + 1, ph, w))
            for n in range(2 * f + 1):
                rows = rows + delta[:, :, n:n + w]
            column = np.zeros((2 * r + 1, h, w))
            for n in range(2 * f + 1):
                column = column + rows[:, n:n + h, :]
            dist = column / taps
            t = 1.0 / (1.0 + 0.25 * np.where(dist < 0.0, 0.0, dist))
            t2 = t * t
            weight = t2 * t2
            for ox in range(-r, r + 1):
                wgt = np.ones((h, w)) if (ox == 0 and oy == 0) else weight[ox + r]
                sum_w = sum_w + wgt
                sum_c = sum_c + wgt[..., None] * se[r + oy:r + oy + h, r + ox:r + ox + w]
        return sum_c / sum_w[..., None]


def denoise_nlm(half_a, half_b, var_a=None, var_b=None, search_radius=0, patch_radius=0, k=0.0):
    """The contract of rttnw_denoise_nlm restated: a dict of the five outputs."""
    a, b = np.asarray(half_a, dtype=np.float64), np.asarray(half_b, dtype=np.float64)
    r, f = search_radius or DEFAULTS["search_radius"], patch_radius or DEFAULTS["patch_radius"]
    kk = k or DEFAULTS["k"]
    k2 = kk * kk
    if var_a is None:
        var_a = var_b = pair_variance(a, b)
    fa = _cross_filter(b, np.asarray(var_b, dtype=np.float64), a, r, f, k2)
    fb = _cross_filter(a, np.asarray(var_a, dtype=np.float64), b, r, f, k2)
    with np.errstate(all="ignore"):
        out = (fa + fb) * 0.5
        d = fa - fb
        return {"linear": out, "rgba8": quantise(out), "half_a": fa, "half_b": fb, "error": (d * d) * 0.25}


def random_inputs(rng, w, h, with_variance=True):
    """Two noisy halves of one image with flat regions, an edge, a texture and fireflies; variances that follow the noise, some of them
    exactly 0 (where only the 1e-10 keeps the distance's denominator positive).  Everything finite."""
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([0.2 + 0.6 * (xx > w // 2), 0.5 + 0.4 * np.sin(0.9 * xx + 0.5 * yy), 0.1 + 0.02 * yy], axis=-1)
    sigma = 0.05 + 0.25 * base * rng.random((h, w, 1))
    halves = []
    for _ in range(2):
        c = base + sigma * rng.standard_normal((h, w, 3)) + (rng.random((h, w, 3)) < 0.02) * rng.exponential(20.0, size=(h, w, 3))
        halves.append(np.abs(c))
    if not with_variance:
        return halves[0], halves[1], None, None
    variances = []
    for _ in range(2):
        v = sigma ** 2 * rng.exponential(1.0, size=(h, w, 3))
        v[rng.random((h, w)) < 0.05] = 0.0
        variances.append(v)
    return halves[0], halves[1], variances[0], variances[1]
