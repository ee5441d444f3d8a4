"""TEST INFRASTRUCTURE for rttnw_temporal_accumulate: a numpy restatement of the contract in include/rttnw_hip.h (not of
rttnw_amd/csrc/temporal.hpp), and the loader of the host build of that header (tests/temporal_host).  The contract's arithmetic starts from the
two camera records, so the restatement takes them from the host's Camera::new (th_camera_record) and restates everything after them.  numpy's
element-wise double arithmetic is IEEE and fuses nothing, and every sum below adds its terms one at a time in the header's order, so the three
— device, host build, this file — must agree bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np

from denoise_ref import quantise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = {"max_history": 32, "depth_tolerance": 0.05, "normal_min": 0.9}
OUTPUTS = ("linear", "rgba8", "variance", "length", "prev_xy")
_LIB = []


def _lib():
    if not _LIB:
        subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "temporal_host"), "-s"], check=True)
        lib = C.CDLL(os.path.join(ROOT, "tests", "temporal_host", "libtemporal_host.so"))
        lib.th_camera_record.argtypes = [C.c_void_p, C.c_void_p]
        lib.th_camera_record.restype = None
        lib.th_temporal_accumulate.argtypes = [C.c_uint32, C.c_uint32] + [C.c_void_p] * 13 + [C.c_uint32, C.c_double, C.c_double] + [C.c_void_p] * 5
        lib.th_temporal_accumulate.restype = C.c_int
        _LIB.append(lib)
    return _LIB[0]


def camera_record(cam):
    """(o, llc, H, V) of a camera descriptor: Camera::new as the library's host half runs it."""
    rec = np.zeros(12)
    _lib().th_camera_record(C.addressof(cam), rec.ctypes.data)
    return rec[0:3], rec[3:6], rec[6:9], rec[9:12]


def _arrays(linear, features, history, variance):
    lin = np.ascontiguousarray(linear, dtype=np.float64)
    f = [np.ascontiguousarray(features[k], dtype=np.float64) for k in ("normal", "depth", "alpha")]
    var = None if variance is None else np.ascontiguousarray(variance, dtype=np.float64)
    prev = [None] * 6
    if history is not None:
        pf = history["features"]
        prev = [None if a is None else np.ascontiguousarray(a, dtype=np.float64)
                for a in (history["linear"], history.get("variance"), history["length"], pf["normal"], pf["depth"], pf["alpha"])]
    return lin, var, f, prev


def host():
    """th_temporal_accumulate of tests/temporal_host, wrapped: the arguments of `accumulate` below -> dict of the outputs, with the frame's
    features and camera beside them, so that a result is the next call's history."""
    lib = _lib()

    def run(linear, features, cam, history=None, variance=None, max_history=0, depth_tolerance=0.0, normal_min=0.0):
        lin, var, f, prev = _arrays(linear, features, history, variance)
        h, w = lin.shape[:2]
        out = {"linear": np.zeros((h, w, 3)), "rgba8": np.zeros((h, w, 4), dtype=np.uint8), "variance": None if var is None else np.zeros((h, w, 3)),
               "length": np.zeros((h, w)), "prev_xy": np.zeros((h, w, 2))}
        ptr = lambda a: None if a is None else a.ctypes.data
        rc = lib.th_temporal_accumulate(w, h, C.addressof(cam), None if history is None else C.addressof(history["cam"]), ptr(lin), ptr(var),
                                        *[ptr(a) for a in f], *[ptr(a) for a in prev], max_history, depth_tolerance, normal_min,
                                        *[ptr(out[name]) for name in OUTPUTS])
        assert rc == 0
        out["features"], out["cam"] = features, cam
        return out
    return run


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def where_it_was(w, h, cam, prev_cam, depth, alpha):
    """Steps 1 and 2 of the contract: (fx, fy, zq, ok) per pixel — ok where the pixel hit something and lies inside the previous frame."""
    ys, xs = np.mgrid[0:h, 0:w]
    hit = alpha != 0.0
    with np.errstate(all="ignore"):
        z = depth / alpha
        if bytes(cam) == bytes(prev_cam):
            return xs.astype(np.float64), ys.astype(np.float64), z, hit
        o, llc, H, V = camera_record(cam)
        op, llcp, Hp, Vp = camera_record(prev_cam)
        s = ((xs.astype(np.float64) + 0.5) / float(w))[..., None]
        t = (((h - 1 - ys).astype(np.float64) + 0.5) / float(h))[..., None]
        d = ((llc + s * H) + t * V) - o
        P = o + d * (z / np.sqrt(_dot(d, d)))[..., None]
        q = P - op
        n = np.array([Hp[1] * Vp[2] - Hp[2] * Vp[1], Hp[2] * Vp[0] - Hp[0] * Vp[2], Hp[0] * Vp[1] - Hp[1] * Vp[0]])
        e = llcp - op
        lam = _dot(e, n) / _dot(q, n)
        r = lam[..., None] * q - e
        sp, tp = _dot(r, Hp) / _dot(Hp, Hp), _dot(r, Vp) / _dot(Vp, Vp)
        fx = sp * float(w) - 0.5
        fy = (float(h) - tp * float(h)) - 0.5
        zq = np.sqrt(_dot(q, q))
        ok = hit & (lam > 0.0) & np.isfinite(fx) & np.isfinite(fy) & (fx > -1.0) & (fx < float(w)) & (fy > -1.0) & (fy < float(h))
    return fx, fy, zq, ok


def tap_acceptance(fx, fy, zq, ok, normal, prev, depth_tolerance=0.0, normal_min=0.0):
    """Step 3: for the taps in the order 00, 10, 01, 11 — (accepted, weight, (rows, columns) clamped into the image)."""
    _, _, plen, pnormal, pdepth, palpha = prev
    h, w = zq.shape
    tol = DEFAULTS["depth_tolerance"] if depth_tolerance == 0.0 else depth_tolerance
    nmin = DEFAULTS["normal_min"] if normal_min == 0.0 else normal_min
    fx, fy = np.where(ok, fx, 0.0), np.where(ok, fy, 0.0)
    x0, y0 = np.floor(fx), np.floor(fy)
    ax, ay = fx - x0, fy - y0
    ix, iy = x0.astype(np.int64), y0.astype(np.int64)
    taps = []
    for j in (0, 1):
        for i in (0, 1):
            tx, ty = ix + i, iy + j
            acc = ok & (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
            cy, cx = np.clip(ty, 0, h - 1), np.clip(tx, 0, w - 1)
            pa = palpha[cy, cx]
            with np.errstate(all="ignore"):
                acc = acc & (pa != 0.0) & (plen[cy, cx] > 0.0) & (np.abs(pdepth[cy, cx] / pa - zq) <= tol * zq)
                if normal_min != -1.0:
                    pn = pnormal[cy, cx]
                    acc = acc & (_dot(normal, pn) >= nmin * np.sqrt(_dot(normal, normal) * _dot(pn, pn)))
            taps.append((acc, (ax if i else 1.0 - ax) * (ay if j else 1.0 - ay), (cy, cx)))
    return taps


def accumulate(linear, features, cam, history=None, variance=None, max_history=0, depth_tolerance=0.0, normal_min=0.0):
    """The contract of rttnw_temporal_accumulate restated: dict of OUTPUTS, and the frame's features and camera beside them."""
    cur, var, (normal, depth, alpha), prev = _arrays(linear, features, history, variance)
    h, w = cur.shape[:2]
    out = {"linear": cur.copy(), "variance": None if var is None else var.copy(), "length": np.ones((h, w)), "prev_xy": np.full((h, w, 2), np.nan),
           "features": features, "cam": cam}
    if history is not None:
        fx, fy, zq, ok = where_it_was(w, h, cam, history["cam"], depth, alpha)
        out["prev_xy"][ok] = np.stack([fx, fy], axis=-1)[ok]
        sw, sl, sc, sv = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w, 3)), np.zeros((h, w, 3))
        with np.errstate(all="ignore"):
            for acc, wt, at in tap_acceptance(fx, fy, zq, ok, normal, prev, depth_tolerance, normal_min):
                sw = np.where(acc, sw + wt, sw)
                sl = np.where(acc, sl + wt * prev[2][at], sl)
                sc = np.where(acc[..., None], sc + wt[..., None] * prev[0][at], sc)
                if var is not None:
                    sv = np.where(acc[..., None], sv + wt[..., None] * prev[1][at], sv)
            blend = ok & (sw > 0.0)
            grown = sl / sw + 1.0
            most = float(max_history or DEFAULTS["max_history"])
            n = np.where(grown < most, grown, most)
            a = 1.0 / n
            b = 1.0 - a
            lin = b[..., None] * (sc / sw[..., None]) + a[..., None] * cur
            out["linear"][blend] = lin[blend]
            out["length"][blend] = n[blend]
            if var is not None:
                v = (b * b)[..., None] * (sv / sw[..., None]) + (a * a)[..., None] * var
                out["variance"][blend] = v[blend]
    out["rgba8"] = quantise(out["linear"])
    return out
