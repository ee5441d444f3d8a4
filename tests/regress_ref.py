"""TEST INFRASTRUCTURE for rttnw_denoise_regress: a numpy restatement of the filter, written from the contract in include/rttnw_hip.h (not from
rttnw_amd/csrc/regress.hpp), and the loader of the host build of that header (tests/regress_host).  Vectorised over the pixels, with explicit
loops over the offsets and over the at most 7x7 indices of the normal equations; numpy's element-wise double arithmetic is IEEE and fuses
nothing, and every sum adds its terms one at a time in the header's order, so the three — device, host build, this file — must agree bit for
bit.  The weights are rttnw_denoise_nlm's: tests/nlm_ref.py's expressions, evaluated one row of offsets at a time."""
import ctypes as C
import os
import subprocess

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from denoise_ref import quantise
from nlm_ref import _extend, pair_variance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = {"search_radius": 7, "patch_radius": 3, "k": 0.7, "ridge": 1e-1}
OUTPUTS = ("linear", "rgba8", "half_a", "half_b", "error", "fit")
FEATURES = ("albedo", "normal", "depth", "alpha")
ALBEDO_EPS = 1e-3


def host():
    """rh_denoise_regress of tests/regress_host, wrapped: (half_a, half_b, var_a or None, var_b or None, features dict or None, ...) -> dict of
    the six outputs."""
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "regress_host"), "-s"], check=True)
    lib = C.CDLL(os.path.join(ROOT, "tests", "regress_host", "libregress_host.so"))
    lib.rh_denoise_regress.argtypes = ([C.c_uint32, C.c_uint32] + [C.c_void_p] * 8 + [C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_uint32, C.c_uint32] +
                                       [C.c_void_p] * 6)
    lib.rh_denoise_regress.restype = C.c_int

    def run(half_a, half_b, var_a=None, var_b=None, features=None, mask=7, demodulate=True, ridge=0.0, search_radius=0, patch_radius=0, k=0.0):
        f = features or {}
        arrs = [None if x is None else np.ascontiguousarray(x, dtype=np.float64) for x in (half_a, half_b, var_a, var_b) + tuple(f.get(n) for n in FEATURES)]
        h, w = arrs[0].shape[:2]
        out = empty_outputs(h, w)
        rc = lib.rh_denoise_regress(w, h, *[None if x is None else x.ctypes.data for x in arrs], search_radius, patch_radius, k, ridge, mask,
                                    1 if demodulate else 0, *[out[name].ctypes.data for name in OUTPUTS])
        assert rc == 0
        return out
    return run


def empty_outputs(h, w):
    return {"linear": np.zeros((h, w, 3)), "rgba8": np.zeros((h, w, 4), dtype=np.uint8), "half_a": np.zeros((h, w, 3)), "half_b": np.zeros((h, w, 3)),
            "error": np.zeros((h, w, 3)), "fit": np.zeros((h, w))}


def _weights(guide, var, r, f, k2):
    """rttnw_denoise_nlm's w(p, o), one offset after the other, row-major: yields (oy, ox, HxW)."""
    h, w = guide.shape[:2]
    ph, pw = h + 2 * f, w + 2 * f
    ge, ve = _extend(guide, r + f), _extend(var, r + f)
    gx, vx = ge[r:r + ph, r:r + pw][None], ve[r:r + ph, r:r + pw][None]
    taps = float(3 * (2 * f + 1) ** 2)
    for oy in range(-r, r + 1):
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
            yield oy, ox, (np.ones((h, w)) if (ox == 0 and oy == 0) else weight[ox + r])


def _components(features, mask):
    """The selected feature components as stored, HxWxd, in the order albedo r g b, normal x y z, depth (as z = depth / alpha)."""
    planes = []
    if mask & 1:
        planes += [features["albedo"][..., c] for c in range(3)]
    if mask & 2:
        planes += [features["normal"][..., c] for c in range(3)]
    if mask & 4:
        planes += [features["depth"] / features["alpha"]]
    return np.stack(planes, axis=-1)


def _cross_regress(guide, var, src, features, mask, r, f, k2, ridge):
    """`src` regressed on the features with the weights found in `guide` (variance `var`): (HxWx3 value, HxW bool "first-order value used")."""
    h, w = guide.shape[:2]
    se = _extend(src, r)
    s, t = np.zeros((h, w)), np.zeros((h, w, 3))
    first = np.zeros((h, w), dtype=bool)
    d = 0
    if mask:
        alpha = np.asarray(features["alpha"], dtype=np.float64)
        first = alpha != 0.0                                          # the pixel's mask m is `mask`; elsewhere it is 0
        comp = _components(features, mask)
        d = comp.shape[-1]
        ce, ae = _extend(comp, r), _extend(alpha, r)
        b = [np.zeros((h, w)) for _ in range(d)]
        A = [[np.zeros((h, w)) for _ in range(i + 1)] for i in range(d)]
        Cm = [[np.zeros((h, w)) for _ in range(3)] for _ in range(d)]
    for oy, ox, wgt in _weights(guide, var, r, f, k2):
        y = se[r + oy:r + oy + h, r + ox:r + ox + w]
        if not mask:
            s = s + wgt
            t = t + wgt[..., None] * y
            continue
        kept = ~first | (ae[r + oy:r + oy + h, r + ox:r + ox + w] != 0.0)   # with m != 0 a candidate with alpha == 0 enters no sum
        s = np.where(kept, s + wgt, s)
        t = np.where(kept[..., None], t + wgt[..., None] * y, t)
        upd = first & kept
        cq = ce[r + oy:r + oy + h, r + ox:r + ox + w]
        x = [cq[..., i] - comp[..., i] for i in range(d)]
        if mask & 4:
            x[d - 1] = x[d - 1] / comp[..., d - 1]                          # (z_q - z_p) / z_p
        for i in range(d):
            wx = wgt * x[i]
            b[i] = np.where(upd, b[i] + wx, b[i])
            for j in range(i + 1):
                A[i][j] = np.where(upd, A[i][j] + wx * x[j], A[i][j])
            for c in range(3):
                Cm[i][c] = np.where(upd, Cm[i][c] + wx * y[..., c], Cm[i][c])
    uu, uG = np.zeros((h, w)), [np.zeros((h, w)) for _ in range(3)]
    ok = np.ones((h, w), dtype=bool)
    if d:
        pivots = np.ones((h, w), dtype=bool)
        rs = ridge * s
        for i in range(d):
            A[i][i] = A[i][i] + rs
        L = [[None] * d for _ in range(d)]
        for j in range(d):
            for i in range(j + 1):
                acc = A[j][i]
                for k in range(i):
                    acc = acc - L[j][k] * L[i][k]
                if i < j:
                    L[j][i] = acc / L[i][i]
                else:
                    pivots &= acc > 0.0
                    L[j][j] = np.sqrt(acc)
        u, G = [None] * d, [[None] * 3 for _ in range(d)]
        for j in range(d):
            acc = np.zeros((h, w))
            for k in range(j):
                acc = acc + L[j][k] * u[k]
            u[j] = (b[j] - acc) / L[j][j]
            for c in range(3):
                acc = np.zeros((h, w))
                for k in range(j):
                    acc = acc + L[j][k] * G[k][c]
                G[j][c] = (Cm[j][c] - acc) / L[j][j]
        uu1, uG1 = np.zeros((h, w)), [np.zeros((h, w)) for _ in range(3)]
        for j in range(d):
            uu1 = uu1 + u[j] * u[j]
            for c in range(3):
                uG1[c] = uG1[c] + u[j] * G[j][c]
        uu = np.where(first, uu1, 0.0)
        uG = [np.where(first, uG1[c], 0.0) for c in range(3)]
        ok = ~first | pivots
    den = s - uu
    ok = ok & (den >= 0.5)
    value = np.stack([np.where(ok, (t[..., c] - uG[c]) / den, t[..., c] / s) for c in range(3)], axis=-1)
    return value, ok


def denoise_regress(half_a, half_b, var_a=None, var_b=None, features=None, mask=7, demodulate=True, ridge=0.0, search_radius=0, patch_radius=0, k=0.0):
    """The contract of rttnw_denoise_regress restated: a dict of the six outputs."""
    a, b = np.asarray(half_a, dtype=np.float64), np.asarray(half_b, dtype=np.float64)
    r, f = search_radius or DEFAULTS["search_radius"], patch_radius or DEFAULTS["patch_radius"]
    kk = k or DEFAULTS["k"]
    k2 = kk * kk
    lam = ridge or DEFAULTS["ridge"]
    with np.errstate(all="ignore"):
        if demodulate:
            albedo = np.asarray(features["albedo"], dtype=np.float64)
            on = (np.asarray(features["alpha"])[..., None] != 0.0) & (albedo > ALBEDO_EPS)
            a, b = np.where(on, a / albedo, a), np.where(on, b / albedo, b)
            if var_a is not None:
                var_a, var_b = np.where(on, var_a / (albedo * albedo), var_a), np.where(on, var_b / (albedo * albedo), var_b)
        if var_a is None:
            var_a = var_b = pair_variance(a, b)
        fa, fit_a = _cross_regress(b, np.asarray(var_b, dtype=np.float64), a, features, mask, r, f, k2, lam)
        fb, fit_b = _cross_regress(a, np.asarray(var_a, dtype=np.float64), b, features, mask, r, f, k2, lam)
        if demodulate:
            fa, fb = np.where(on, fa * albedo, fa), np.where(on, fb * albedo, fb)
        out = (fa + fb) * 0.5
        d = fa - fb
        return {"linear": out, "rgba8": quantise(out), "half_a": fa, "half_b": fb, "error": (d * d) * 0.25,
                "fit": fit_a.astype(np.float64) + fit_b.astype(np.float64)}


def random_features(rng, w, h):
    """Feature maps as rttnw_render_features makes them: an albedo with a texture and some channels at or under the demodulation threshold, sample-mean
    normals (shorter than 1 in places), fractional alphas on silhouettes, a sky region with alpha 0, depth = z * alpha with z in [1, 10] and a
    step in it."""
    yy, xx = np.mgrid[0:h, 0:w]
    albedo = 0.2 + 0.8 * rng.random((h, w, 3))
    albedo[rng.random((h, w)) < 0.04, 1] = 0.0
    albedo[rng.random((h, w)) < 0.02] = 1e-3
    normal = rng.standard_normal((h, w, 3))
    normal /= np.linalg.norm(normal, axis=-1, keepdims=True)
    normal *= np.where(rng.random((h, w, 1)) < 0.2, 0.7, 1.0)
    alpha = np.ones((h, w))
    alpha[rng.random((h, w)) < 0.1] = 0.5
    alpha[(xx + 2 * yy) % 13 == 0] = 0.0
    if h > 4 and w > 4:
        alpha[:2, -3:] = 0.0
    z = 1.0 + 4.0 * rng.random((h, w)) + 5.0 * (xx > w // 3)
    return {"albedo": albedo, "normal": normal, "depth": z * alpha, "alpha": alpha}
