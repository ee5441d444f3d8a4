"""TEST INFRASTRUCTURE for rttnw_svgf_push / rttnw_svgf_frame: the contract of include/rttnw_hip.h restated as what it says it is — a composition
of the restatements of rttnw_temporal_variance (variance_ref.estimate), rttnw_temporal_accumulate (temporal_ref.accumulate) and rttnw_denoise
(denoise_ref.denoise), plus the demodulation — and the loader of the host build of rttnw_amd/csrc/svgf.hpp (tests/svgf_host).  An
implementation is a class Sequence(width, height, **SETTINGS) with push(linear, features, cam) -> dict of OUTPUTS, reset() and, for the two on
the host, load(state) to start from a made-up history; rttnw_amd.render.SvgfSequence has the same push and reset."""
import ctypes as C
import os
import subprocess

import numpy as np

import denoise_ref
import temporal_ref
import variance_ref
from rttnw_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("linear_rgb", "rgba8", "accumulated_rgb", "variance_rgb", "filtered_variance_rgb", "length", "prev_xy", "moment1_rgb", "moment2_rgb",
           "history_rgb", "raw_rgb", "albedo", "normal", "depth", "alpha")
CHANNELS = {"linear_rgb": 3, "rgba8": 4, "accumulated_rgb": 3, "variance_rgb": 3, "filtered_variance_rgb": 3, "length": 0, "prev_xy": 2,
            "moment1_rgb": 3, "moment2_rgb": 3, "history_rgb": 3, "raw_rgb": 3, "albedo": 3, "normal": 3, "depth": 0, "alpha": 0}
SETTINGS = dict(feedback=0, demodulate=False, iterations=5, sigma_luminance=0.0, sigma_normal=0.0, sigma_depth=0.0, max_history=0, depth_tolerance=0.0,
                normal_min=0.0, min_temporal=0, radius=0, variance_sigma_normal=0.0, variance_sigma_depth=0.0)
ALBEDO_EPS = 1e-3
_LIB = []


def _settings(kw):
    unknown = set(kw) - set(SETTINGS)
    assert not unknown, unknown
    return dict(SETTINGS, **kw)


def _state_of(out, features, cam):
    """What the next call reprojects: a call's outputs as its successor's state."""
    return {"H": out["history_rgb"], "M1": out["moment1_rgb"], "M2": out["moment2_rgb"], "L": out["length"], "features": features, "cam": cam}


class Restated:
    """The composition, step by step as the header numbers them."""

    def __init__(self, width, height, **kw):
        self.width, self.height, self.s, self.state = width, height, _settings(kw), None

    def reset(self):
        self.state = None

    def load(self, state):
        self.state = state

    def push(self, linear, features, cam):
        s, st = self.s, self.state
        C_ = np.ascontiguousarray(linear, dtype=np.float64)
        F = {k: np.ascontiguousarray(features[k], dtype=np.float64) for k in ("albedo", "normal", "depth", "alpha")}
        assert C_.shape == (self.height, self.width, 3)
        # 0
        divided = np.zeros(C_.shape, dtype=bool)
        c, A1 = C_, F["albedo"]
        if s["demodulate"]:
            divided = (F["alpha"][..., None] != 0.0) & (F["albedo"] > ALBEDO_EPS)
            with np.errstate(all="ignore"):
                c = np.where(divided, C_ / F["albedo"], C_)
            A1 = np.ones_like(C_)
        # 1
        t = dict(max_history=s["max_history"], depth_tolerance=s["depth_tolerance"], normal_min=s["normal_min"])
        history = None if st is None else {"linear": st["M1"], "moment2": st["M2"], "length": st["L"], "features": st["features"], "cam": st["cam"]}
        TV = variance_ref.estimate(c, F, cam, history=history, min_temporal=s["min_temporal"], radius=s["radius"], sigma_normal=s["variance_sigma_normal"],
                                   sigma_depth=s["variance_sigma_depth"], **t)
        # 2
        A = TV["linear"]
        if s["feedback"] > 0 and st is not None:
            over_h = temporal_ref.accumulate(c, F, cam, history={"linear": st["H"], "variance": None, "length": st["L"], "features": st["features"],
                                                                 "cam": st["cam"]}, **t)
            assert np.array_equal(over_h["length"], TV["length"]) and np.array_equal(over_h["prev_xy"], TV["prev_xy"], equal_nan=True)
            A = over_h["linear"]
        # 3, 4
        F1 = dict(F, albedo=A1)
        sig = dict(sigma_luminance=s["sigma_luminance"], sigma_normal=s["sigma_normal"], sigma_depth=s["sigma_depth"])
        D, _, Dv = denoise_ref.denoise(A, TV["variance"], F1, s["iterations"], **sig)
        H = denoise_ref.denoise(A, TV["variance"], F1, s["feedback"], **sig)[0] if s["feedback"] > 0 else TV["linear"]
        # 5
        with np.errstate(all="ignore"):
            shown = np.where(divided, D * F["albedo"], D)
            accumulated = np.where(divided, A * F["albedo"], A)
        out = {"linear_rgb": shown, "rgba8": denoise_ref.quantise(shown), "accumulated_rgb": accumulated, "variance_rgb": TV["variance"],
               "filtered_variance_rgb": Dv, "length": TV["length"], "prev_xy": TV["prev_xy"], "moment1_rgb": TV["linear"], "moment2_rgb": TV["moment2"],
               "history_rgb": H, "raw_rgb": C_, "albedo": F["albedo"], "normal": F["normal"], "depth": F["depth"], "alpha": F["alpha"]}
        self.state = _state_of(out, F, cam)
        return out


def params_of(s):
    """The rttnw_svgf_params of a dict of SETTINGS."""
    return abi.Svgf(feedback_iterations=int(s["feedback"]), demodulate=1 if s["demodulate"] else 0, feature_spp=0, reserved0=0,
                    t=abi.Temporal(max_history=s["max_history"], reserved0=0, depth_tolerance=s["depth_tolerance"], normal_min=s["normal_min"]),
                    v=abi.Variance(min_temporal=s["min_temporal"], radius=s["radius"], sigma_normal=s["variance_sigma_normal"],
                                   sigma_depth=s["variance_sigma_depth"], reserved0=0, reserved1=0),
                    d=abi.Denoise(iterations=s["iterations"], reserved0=0, sigma_luminance=s["sigma_luminance"], sigma_normal=s["sigma_normal"],
                                  sigma_depth=s["sigma_depth"]))


def empty_outputs(h, w):
    return {name: np.zeros((h, w, CHANNELS[name]) if CHANNELS[name] else (h, w), dtype=np.uint8 if name == "rgba8" else np.float64) for name in OUTPUTS}


def _lib():
    if not _LIB:
        subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "svgf_host"), "-s"], check=True)
        lib = C.CDLL(os.path.join(ROOT, "tests", "svgf_host", "libsvgf_host.so"))
        lib.sh_svgf_push.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(abi.Svgf)] + [C.c_void_p] * 14 + [C.POINTER(abi.SvgfOut)]
        lib.sh_svgf_push.restype = C.c_int
        _LIB.append(lib)
    return _LIB[0]


class Host:
    """sh_svgf_push of tests/svgf_host, with the state kept here between the calls."""

    def __init__(self, width, height, **kw):
        self.width, self.height, self.s, self.state, self.lib = width, height, _settings(kw), None, _lib()

    def reset(self):
        self.state = None

    def load(self, state):
        self.state = state

    def push(self, linear, features, cam, no_outputs=False):
        st, h, w = self.state, self.height, self.width
        lin = np.ascontiguousarray(linear, dtype=np.float64)
        f = [np.ascontiguousarray(features[k], dtype=np.float64) for k in ("albedo", "normal", "depth", "alpha")]
        prev = [None] * 7
        if st is not None:
            pf = st["features"]
            prev = [np.ascontiguousarray(a, dtype=np.float64) for a in (st["M1"], st["M2"], st["H"], st["L"], pf["normal"], pf["depth"], pf["alpha"])]
        arrays = empty_outputs(h, w)
        out = abi.SvgfOut(image_ms=None, **{name: a.ctypes.data for name, a in arrays.items()})
        q = params_of(self.s)
        ptr = lambda a: None if a is None else a.ctypes.data
        rc = self.lib.sh_svgf_push(w, h, C.byref(q), C.addressof(cam), None if st is None else C.addressof(st["cam"]), ptr(lin), *[ptr(a) for a in f],
                                   *[ptr(a) for a in prev], C.byref(out))
        assert rc == 0
        self.state = _state_of(arrays, dict(zip(("albedo", "normal", "depth", "alpha"), f)), cam)
        return arrays
