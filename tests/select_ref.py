"""TEST INFRASTRUCTURE for rttnw_denoise_select: a numpy restatement of steps 3 to 6 of the contract in include/rttnw_hip.h (not of
rttnw_amd/csrc/select.hpp) over the numpy restatements of the two filters (denoise_ref.denoise, nlm_ref.denoise_nlm), and the loader of the host
build of that header (tests/select_host).  numpy's element-wise double arithmetic is IEEE and fuses nothing, and every sum below adds its terms
one at a time in the header's order, so the three — device, host build, this file — must agree bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np

import denoise_ref
import nlm_ref
from denoise_ref import quantise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = {"error_radius": 5, "blend_radius": 2, "margin": 0.01}
OUTPUTS = ("linear", "rgba8", "blend", "feature", "nlm", "error")


def _empty_outputs(h, w):
    return {"linear": np.zeros((h, w, 3)), "rgba8": np.zeros((h, w, 4), dtype=np.uint8), "blend": np.zeros((h, w)), "feature": np.zeros((h, w, 3)),
            "nlm": np.zeros((h, w, 3)), "error": np.zeros((h, w, 3))}


def host():
    """sh_denoise_select of tests/select_host, wrapped: the arguments of `denoise_select` below -> dict of the six outputs."""
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "select_host"), "-s"], check=True)
    lib = C.CDLL(os.path.join(ROOT, "tests", "select_host", "libselect_host.so"))
    lib.sh_denoise_select.argtypes = ([C.c_uint32, C.c_uint32] + [C.c_void_p] * 8 + [C.c_uint32, C.c_double, C.c_double, C.c_double] +
                                      [C.c_uint32, C.c_uint32, C.c_double] + [C.c_uint32, C.c_uint32, C.c_double, C.c_uint32] + [C.c_void_p] * 6)
    lib.sh_denoise_select.restype = C.c_int

    def run(half_a, half_b, f, var_a=None, var_b=None, iterations=5, search_radius=0, patch_radius=0, k=0.0, error_radius=0, blend_radius=0, margin=None):
        arrs = [None if x is None else np.ascontiguousarray(x, dtype=np.float64)
                for x in (half_a, half_b, var_a, var_b, f["albedo"], f["normal"], f["depth"], f["alpha"])]
        h, w = arrs[0].shape[:2]
        out = _empty_outputs(h, w)
        rc = lib.sh_denoise_select(w, h, *[None if x is None else x.ctypes.data for x in arrs], iterations, 0.0, 0.0, 0.0, search_radius, patch_radius, k,
                                   error_radius, blend_radius, 0.0 if margin is None else margin, 1 if margin is None else 0,
                                   *[out[name].ctypes.data for name in OUTPUTS])
        assert rc == 0
        return out
    return run


def filtered_halves(half_a, half_b, f, var_a=None, var_b=None, iterations=5, search_radius=0, patch_radius=0, k=0.0):
    """Steps 1 and 2: (Fa, Fb, Na, Nb) from the numpy restatements of the two filters."""
    fa = denoise_ref.denoise(half_a, var_a, f, iterations)[0]
    fb = denoise_ref.denoise(half_b, var_b, f, iterations)[0]
    nl = nlm_ref.denoise_nlm(half_a, half_b, var_a, var_b, search_radius, patch_radius, k)
    return fa, fb, nl["half_a"], nl["half_b"]


def _window_sums(v, radius):
    """The two-stage clamped sum: rows left to right, then columns top to bottom, each from 0.0."""
    h, w = v.shape
    e = np.pad(v, ((0, 0), (radius, radius)), mode="edge")
    rows = np.zeros((h, w))
    for n in range(2 * radius + 1):
        rows = rows + e[:, n:n + w]
    e = np.pad(rows, ((radius, radius), (0, 0)), mode="edge")
    out = np.zeros((h, w))
    for n in range(2 * radius + 1):
        out = out + e[n:n + h, :]
    return out


def _blend(beta, n, f):
    b = beta[..., None] if n.ndim == 3 else beta
    with np.errstate(all="ignore"):
        mixed = b * n + (1.0 - b) * f
    return np.where(b == 0.0, f, np.where(b == 1.0, n, mixed))


def select(half_a, half_b, fa, fb, na, nb, error_radius=0, blend_radius=0, margin=None):
    """Steps 3 to 6 of the contract restated: a dict of the six outputs."""
    a, b = np.asarray(half_a, dtype=np.float64), np.asarray(half_b, dtype=np.float64)
    s, t = error_radius or DEFAULTS["error_radius"], blend_radius or DEFAULTS["blend_radius"]
    tau = DEFAULTS["margin"] if margin is None else margin
    with np.errstate(all="ignore"):
        def cross_error(xa, xb):
            term = (xa - b) * (xa - b) + (xb - a) * (xb - a)
            return (term[..., 0] + term[..., 1]) + term[..., 2]
        e_f, e_n = cross_error(fa, fb), cross_error(na, nb)
        d = (e_f - e_n) / (1e-10 + (e_f + e_n))
        m = np.where(_window_sums(d, s) > tau * float((2 * s + 1) ** 2), 1.0, 0.0)
        beta = _window_sums(m, t) / float((2 * t + 1) ** 2)
        feature, nlm = (fa + fb) * 0.5, (na + nb) * 0.5
        out = _blend(beta, nlm, feature)
        diff = _blend(beta, na, fa) - _blend(beta, nb, fb)
        return {"linear": out, "rgba8": quantise(out), "blend": beta, "feature": feature, "nlm": nlm, "error": (diff * diff) * 0.25}


def denoise_select(half_a, half_b, f, var_a=None, var_b=None, iterations=5, search_radius=0, patch_radius=0, k=0.0, error_radius=0, blend_radius=0,
                   margin=None):
    """The contract of rttnw_denoise_select restated: a dict of the six outputs."""
    fa, fb, na, nb = filtered_halves(half_a, half_b, f, var_a, var_b, iterations, search_radius, patch_radius, k)
    return select(half_a, half_b, fa, fb, na, nb, error_radius, blend_radius, margin)


def synthetic_frame(seed, noise=0.15):
    """The 64x48 frame whose truth is known (the issue's table): columns 0-15 and 16-31 are two flat walls whose faint colour edge lies on the
    feature edge, columns 32-63 one surface with stripes the features cannot see.  Returns (half_a, half_b, features, truth)."""
    h, w = 48, 64
    yy, xx = np.mgrid[0:h, 0:w]
    truth = np.zeros((h, w, 3))
    truth[:, :16] = (0.50, 0.45, 0.40)
    truth[:, 16:32] = (0.62, 0.55, 0.48)
    stripe = (((xx + yy) // 4) % 2 == 1)[:, 32:]
    truth[:, 32:] = np.where(stripe[..., None], (0.8, 0.3, 0.2), (0.2, 0.3, 0.8))
    normal = np.zeros((h, w, 3))
    normal[:, :16] = (0.0, 0.0, 1.0)
    normal[:, 16:32] = (1.0, 0.0, 0.0)
    normal[:, 32:] = (0.0, 1.0, 0.0)
    f = {"albedo": np.ones((h, w, 3)), "normal": normal, "depth": np.full((h, w), 5.0), "alpha": np.ones((h, w))}
    rng = np.random.default_rng(seed)
    half_a = truth + noise * np.sqrt(2.0) * truth * rng.standard_normal((h, w, 3))
    half_b = truth + noise * np.sqrt(2.0) * truth * rng.standard_normal((h, w, 3))
    return half_a, half_b, f, truth


def check_synthetic(out, truth):
    """The conditions of the synthetic frame, one seed: on columns 36-63 beta is exactly 1 and the output is N bit for bit; on columns 0-27 the
    mean beta is below 0.5 and the output lies closer to the truth than the geometric mean of the two filters' errors.  Returns the figures."""
    def mse(img, cols):
        return float(np.mean((img[:, cols] - truth[:, cols]) ** 2))
    left, right = slice(0, 28), slice(36, 64)
    fig = {"beta_left": float(out["blend"][:, left].mean()), "beta_right_min": float(out["blend"][:, right].min()),
           "F_left": mse(out["feature"], left), "N_left": mse(out["nlm"], left), "out_left": mse(out["linear"], left),
           "F_right": mse(out["feature"], right), "N_right": mse(out["nlm"], right)}
    fig["ratio"] = fig["out_left"] / np.sqrt(fig["F_left"] * fig["N_left"])
    print("synthetic frame: left MSE F %.3g, N %.3g, output %.3g (%.2f of the geometric mean), mean beta %.3f; right MSE F %.3g, N %.3g, min beta %.3f"
          % (fig["F_left"], fig["N_left"], fig["out_left"], fig["ratio"], fig["beta_left"], fig["F_right"], fig["N_right"], fig["beta_right_min"]))
    assert np.all(out["blend"][:, right] == 1.0), fig
    assert np.array_equal(np.ascontiguousarray(out["linear"][:, right]).view(np.uint8), np.ascontiguousarray(out["nlm"][:, right]).view(np.uint8))
    assert fig["beta_left"] < 0.5, fig
    assert fig["out_left"] < np.sqrt(fig["F_left"] * fig["N_left"]), fig
    return fig
