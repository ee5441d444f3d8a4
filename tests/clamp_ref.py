"""TEST INFRASTRUCTURE for rttnw_temporal_clamp: a numpy restatement of the contract in include/rttnw_hip.h (not of rttnw_amd/csrc/clamp.hpp), and
the loader of the host build of that header (tests/clamp_host).  Stage S is written out here, tap by tap; stage A' follows steps 1 - 3 of
rttnw_temporal_accumulate through that contract's restated steps (temporal_ref.where_it_was, temporal_ref.tap_acceptance) and is written out from
the sums on; stage B is rttnw_temporal_variance's, through variance_ref.  numpy's element-wise double arithmetic is IEEE and fuses nothing, and
every sum below adds its terms one at a time in the header's order, so the three — device, host build, this file — must agree bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np

import temporal_ref
import variance_ref
from denoise_ref import quantise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = {"clamp_radius": 3, "gamma": 1.0, "sigma_normal": 64.0, "sigma_depth": 0.1}
SHARED = variance_ref.OUTPUTS                                  # what rttnw_temporal_variance returns as well
OUTPUTS = SHARED + ("mean", "sd", "clipped")
TINY = 1e-12
_LIB = []


def _lib():
    if not _LIB:
        subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "clamp_host"), "-s"], check=True)
        lib = C.CDLL(os.path.join(ROOT, "tests", "clamp_host", "libclamp_host.so"))
        lib.ch_temporal_clamp.argtypes = ([C.c_uint32, C.c_uint32] + [C.c_void_p] * 12 +
                                          [C.c_uint32, C.c_double, C.c_double, C.c_uint32, C.c_uint32, C.c_double, C.c_double] +
                                          [C.c_uint32, C.c_double, C.c_double, C.c_double] + [C.c_void_p] * 9)
        lib.ch_temporal_clamp.restype = C.c_int
        _LIB.append(lib)
    return _LIB[0]


def empty_outputs(h, w):
    out = variance_ref.empty_outputs(h, w)
    out.update({"mean": np.zeros((h, w, 3)), "sd": np.zeros((h, w, 3)), "clipped": np.zeros((h, w), dtype=np.uint8)})
    return out


def host():
    """ch_temporal_clamp of tests/clamp_host, wrapped: the arguments of `clamp` below -> dict of the outputs, with the frame's features and camera
    beside them, so that a result is the next call's history."""
    lib = _lib()

    def run(linear, features, cam, history=None, gamma=0.0, clamp_radius=0, clamp_sigma_normal=0.0, clamp_sigma_depth=0.0, max_history=0,
            depth_tolerance=0.0, normal_min=0.0, min_temporal=0, radius=0, sigma_normal=0.0, sigma_depth=0.0):
        lin, f, prev = variance_ref._arrays(linear, features, history)
        h, w = lin.shape[:2]
        out = empty_outputs(h, w)
        ptr = lambda a: None if a is None else a.ctypes.data
        rc = lib.ch_temporal_clamp(w, h, C.addressof(cam), None if history is None else C.addressof(history["cam"]), ptr(lin), *[ptr(a) for a in f],
                                   *[ptr(a) for a in prev], max_history, depth_tolerance, normal_min, min_temporal, radius, sigma_normal, sigma_depth,
                                   clamp_radius, gamma, clamp_sigma_normal, clamp_sigma_depth, *[ptr(out[name]) for name in OUTPUTS])
        assert rc == 0
        out["features"], out["cam"] = features, cam
        return out
    return run


def _pos(x):
    return np.where(x < 0.0, 0.0, x)          # a NaN stays a NaN


def _shifted(a, dy, dx):
    """a[y + dy, x + dx] where that lies inside the image (elsewhere the value is never used)."""
    h, w = a.shape[:2]
    ys, xs = np.mgrid[0:h, 0:w]
    return a[np.clip(ys + dy, 0, h - 1), np.clip(xs + dx, 0, w - 1)]


def statistics(cur, normal, depth, alpha, radius, sigma_normal, sigma_depth):
    """Stage S: (mu, sd) of every pixel."""
    h, w = alpha.shape
    ys, xs = np.mgrid[0:h, 0:w]
    squarings = 0
    while squarings < 10 and float(1 << squarings) < sigma_normal:
        squarings += 1
    square = cur * cur                                                      # m2' = cur * cur, rounded once
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
                s1 = np.where(keep[..., None], s1 + wt[..., None] * _shifted(cur, dy, dx), s1)
                s2 = np.where(keep[..., None], s2 + wt[..., None] * _shifted(square, dy, dx), s2)
        some = (sw > 0.0)[..., None]
        mu = np.where(some, s1 / sw[..., None], cur)
        q = np.where(some, s2 / sw[..., None], square)
        sd = np.sqrt(_pos(q - mu * mu))
    miss = (alpha == 0.0)[..., None]
    return np.where(miss, cur, mu), np.where(miss, 0.0, sd)


def clip(h1, lo, hi):
    """(h1c, which of the two branches was taken): h1 < lo ? lo : (h1 > hi ? hi : h1); a comparison with a NaN is false."""
    with np.errstate(all="ignore"):
        below = h1 < lo
        above = ~below & (h1 > hi)
    return np.where(below, lo, np.where(above, hi, h1)), below | above


def clamp(linear, features, cam, history=None, gamma=0.0, clamp_radius=0, clamp_sigma_normal=0.0, clamp_sigma_depth=0.0, max_history=0,
          depth_tolerance=0.0, normal_min=0.0, min_temporal=0, radius=0, sigma_normal=0.0, sigma_depth=0.0):
    """The contract of rttnw_temporal_clamp restated: dict of OUTPUTS, and the frame's features and camera beside them."""  # (and "blended")
    cur, (normal, depth, alpha), prev = variance_ref._arrays(linear, features, history)
    h, w = cur.shape[:2]
    g = float(gamma or DEFAULTS["gamma"])
    mu, sd = statistics(cur, normal, depth, alpha, clamp_radius or DEFAULTS["clamp_radius"], clamp_sigma_normal or DEFAULTS["sigma_normal"],
                        clamp_sigma_depth or DEFAULTS["sigma_depth"])
    square = cur * cur
    m1, m2, length, xy = cur.copy(), square.copy(), np.ones((h, w)), np.full((h, w, 2), np.nan)
    clipped, blend = np.zeros((h, w), dtype=np.uint8), np.zeros((h, w), dtype=bool)
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
            lo, hi = mu - g * sd, mu + g * sd
            h1, h2 = sc / sw[..., None], s2 / sw[..., None]
            h1c, moved = clip(h1, lo, hi)
            h2c = np.where(moved, (h2 - h1 * h1) + h1c * h1c, h2)            # the history keeps its spread about the moved mean
            m1[blend] = (b[..., None] * h1c + a[..., None] * cur)[blend]
            m2[blend] = (b[..., None] * h2c + a[..., None] * square)[blend]
            length[blend] = n[blend]
            bits = (moved[..., 0] * 1 + moved[..., 1] * 2 + moved[..., 2] * 4).astype(np.uint8)
            clipped[blend] = bits[blend]
    trusted = float(min_temporal or variance_ref.DEFAULTS["min_temporal"])
    with np.errstate(all="ignore"):                                            # stage B, rttnw_temporal_variance's, on stage A''s outputs
        temporal = _pos(m2 - m1 * m1) / (length - 1.0)[..., None]
        window = variance_ref.spatial(m1, m2, length, normal, depth, alpha, radius or variance_ref.DEFAULTS["radius"],
                                      sigma_normal or variance_ref.DEFAULTS["sigma_normal"], sigma_depth or variance_ref.DEFAULTS["sigma_depth"])
        var = np.where((length >= trusted)[..., None], temporal, window)
    var = np.where((alpha == 0.0)[..., None], 0.0, var)
    return {"linear": m1, "rgba8": quantise(m1), "moment2": m2, "length": length, "prev_xy": xy, "variance": var, "mean": mu, "sd": sd, "clipped": clipped,
            "features": features, "cam": cam, "blended": blend}               # blended (no output of the call): W > 0, the history was used
