"""TEST INFRASTRUCTURE for rttnw_temporal_variance: a numpy restatement of the contract in include/rttnw_hip.h (not of
rttnw_amd/csrc/variance.hpp), and the loader of the host build of that header (tests/variance_host).  Stage A follows steps 1 - 4 of
rttnw_temporal_accumulate, so it is written over that contract's restated steps (temporal_ref.where_it_was, temporal_ref.tap_acceptance);
stage B is written out here, tap by tap.  numpy's element-wise double arithmetic is IEEE and fuses nothing, and every sum below adds its
terms one at a time in the header's order, so the three — device, host build, this file — must agree bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np

import temporal_ref
from denoise_ref import quantise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = {"min_temporal": 4, "radius": 3, "sigma_normal": 64.0, "sigma_depth": 0.1}
OUTPUTS = ("linear", "rgba8", "moment2", "length", "prev_xy", "variance")
TINY = 1e-12
_LIB = []


def _lib():
    if not _LIB:
        subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "variance_host"), "-s"], check=True)
        lib = C.CDLL(os.path.join(ROOT, "tests", "variance_host", "libvariance_host.so"))
        lib.vh_temporal_variance.argtypes = ([C.c_uint32, C.c_uint32] + [C.c_void_p] * 12 + [C.c_uint32, C.c_double, C.c_double, C.c_uint32, C.c_uint32,
                                                                                             C.c_double, C.c_double] + [C.c_void_p] * 6)
        lib.vh_temporal_variance.restype = C.c_int
        _LIB.append(lib)
    return _LIB[0]


def _arrays(linear, features, history):
    lin = np.ascontiguousarray(linear, dtype=np.float64)
    f = [np.ascontiguousarray(features[k], dtype=np.float64) for k in ("normal", "depth", "alpha")]
    prev = [None] * 6
    if history is not None:
        pf = history["features"]
        prev = [np.ascontiguousarray(a, dtype=np.float64)
                for a in (history["linear"], history["moment2"], history["length"], pf["normal"], pf["depth"], pf["alpha"])]
    return lin, f, prev


def empty_outputs(h, w):
    return {"linear": np.zeros((h, w, 3)), "rgba8": np.zeros((h, w, 4), dtype=np.uint8), "moment2": np.zeros((h, w, 3)), "length": np.zeros((h, w)),
            "prev_xy": np.zeros((h, w, 2)), "variance": np.zeros((h, w, 3))}


def host():
    """vh_temporal_variance of tests/variance_host, wrapped: the arguments of `estimate` below -> dict of the outputs, with the frame's features
    and camera beside them, so that a result is the next call's history."""
    lib = _lib()

    def run(linear, features, cam, history=None, max_history=0, depth_tolerance=0.0, normal_min=0.0, min_temporal=0, radius=0, sigma_normal=0.0,
            sigma_depth=0.0):
        lin, f, prev = _arrays(linear, features, history)
        h, w = lin.shape[:2]
        out = empty_outputs(h, w)
        ptr = lambda a: None if a is None else a.ctypes.data
        rc = lib.vh_temporal_variance(w, h, C.addressof(cam), None if history is None else C.addressof(history["cam"]), ptr(lin), *[ptr(a) for a in f],
                                      *[ptr(a) for a in prev], max_history, depth_tolerance, normal_min, min_temporal, radius, sigma_normal, sigma_depth,
                                      *[ptr(out[name]) for name in OUTPUTS])
        assert rc == 0
        out["features"], out["cam"] = features, cam
        return out
    return run


def accumulate(linear, features, cam, history=None, max_history=0, depth_tolerance=0.0, normal_min=0.0):
    """Stage A: (m1, m2, N, prev_xy)."""
    cur, (normal, depth, alpha), prev = _arrays(linear, features, history)
    h, w = cur.shape[:2]
    square = cur * cur
    m1, m2, length, xy = cur.copy(), square.copy(), np.ones((h, w)), np.full((h, w, 2), np.nan)
    if history is not None:
        fx, fy, zq, ok = temporal_ref.where_it_was(w, h, cam, history["cam"], depth, alpha)
        xy[ok] = np.stack([fx, fy], axis=-1)[ok]
        sw, sl, sc, s2 = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w, 3)), np.zeros((h, w, 3))
        taps_of = [prev[0], None, prev[2], prev[3], prev[4], prev[5]]          # tap_acceptance reads length, normal, depth, alpha
        with np.errstate(all="ignore"):
            for acc, wt, at in temporal_ref.tap_acceptance(fx, fy, zq, ok, normal, taps_of, depth_tolerance, normal_min):
                sw = np.where(acc, sw + wt, sw)
                sl = np.where(acc, sl + wt * prev[2][at], sl)
                sc = np.where(acc[..., None], sc + wt[..., None] * prev[0][at], sc)
                s2 = np.where(acc[..., None], s2 + wt[..., None] * prev[1][at], s2)
            blend = ok & (sw > 0.0)
            grown = sl / sw + 1.0
            most = float(max_history or temporal_ref.DEFAULTS["max_history"])
            n = np.where(grown < most, grown, most)
            a = 1.0 / n
            b = 1.0 - a
            m1[blend] = (b[..., None] * (sc / sw[..., None]) + a[..., None] * cur)[blend]
            m2[blend] = (b[..., None] * (s2 / sw[..., None]) + a[..., None] * square)[blend]
            length[blend] = n[blend]
    return m1, m2, length, xy


def _pos(x):
    return np.where(x < 0.0, 0.0, x)          # a NaN stays a NaN


def _shifted(a, dy, dx):
    """a[y + dy, x + dx] where that lies inside the image (elsewhere the value is never used)."""
    h, w = a.shape[:2]
    ys, xs = np.mgrid[0:h, 0:w]
    return a[np.clip(ys + dy, 0, h - 1), np.clip(xs + dx, 0, w - 1)]


def spatial(m1, m2, length, normal, depth, alpha, radius, sigma_normal, sigma_depth):
    """The spatial estimate at EVERY pixel (the caller keeps it where it applies)."""
    h, w = length.shape
    ys, xs = np.mgrid[0:h, 0:w]
    squarings = 0
    while squarings < 10 and float(1 << squarings) < sigma_normal:
        squarings += 1
    sw, s1, s2 = np.zeros((h, w)), np.zeros((h, w, 3)), np.zeros((h, w, 3))
    with np.errstate(all="ignore"):
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                inside = (ys + dy >= 0) & (ys + dy < h) & (xs + dx >= 0) & (xs + dx < w)
                keep = inside & (_shifted(alpha, dy, dx) != 0.0)
                n, z = _shifted(normal, dy, dx), _shifted(depth, dy, dx)
                wn = (normal[..., 0] * n[..., 0] + normal[..., 1] * n[..., 1]) + normal[..., 2] * n[..., 2]
                wn = np.where(wn > 0.0, wn, 0.0)
                for _ in range(squarings):
                    wn = wn * wn
                qz = (depth - z) / ((sigma_depth * (np.abs(depth) + np.abs(z))) * 0.5 + TINY)
                r = 1.0 / (1.0 + qz * qz)
                wt = wn * (r * r)
                sw = np.where(keep, sw + wt, sw)
                s1 = np.where(keep[..., None], s1 + wt[..., None] * _shifted(m1, dy, dx), s1)
                s2 = np.where(keep[..., None], s2 + wt[..., None] * _shifted(m2, dy, dx), s2)
        some = (sw > 0.0)[..., None]
        a1 = np.where(some, s1 / sw[..., None], m1)
        a2 = np.where(some, s2 / sw[..., None], m2)
        return _pos(a2 - a1 * a1) / length[..., None]


def estimate(linear, features, cam, history=None, max_history=0, depth_tolerance=0.0, normal_min=0.0, min_temporal=0, radius=0, sigma_normal=0.0,
             sigma_depth=0.0):
    """The contract of rttnw_temporal_variance restated: dict of OUTPUTS, and the frame's features and camera beside them."""
    m1, m2, length, xy = accumulate(linear, features, cam, history, max_history, depth_tolerance, normal_min)
    normal, depth, alpha = (np.ascontiguousarray(features[k], dtype=np.float64) for k in ("normal", "depth", "alpha"))
    trusted = float(min_temporal or DEFAULTS["min_temporal"])
    with np.errstate(all="ignore"):
        temporal = _pos(m2 - m1 * m1) / (length - 1.0)[..., None]
        window = spatial(m1, m2, length, normal, depth, alpha, radius or DEFAULTS["radius"], sigma_normal or DEFAULTS["sigma_normal"],
                         sigma_depth or DEFAULTS["sigma_depth"])
        var = np.where((length >= trusted)[..., None], temporal, window)
    var = np.where((alpha == 0.0)[..., None], 0.0, var)
    return {"linear": m1, "rgba8": quantise(m1), "moment2": m2, "length": length, "prev_xy": xy, "variance": var, "features": features, "cam": cam}
