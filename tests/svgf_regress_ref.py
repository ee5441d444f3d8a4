"""TEST INFRASTRUCTURE for the regression stage of the rttnw_svgf handle (rttnw_svgf_set_regress / _push_halves / _halves): the contract of
include/rttnw_hip.h restated as what it says it is — a composition of the restatements of rttnw_temporal_variance (variance_ref.estimate),
rttnw_temporal_accumulate twice (temporal_ref.accumulate) and rttnw_denoise_regress (regress_ref.denoise_regress), plus the demodulation — the
loader of the host build of rttnw_amd/csrc/svgf.hpp's stage (tests/svgf_regress_host), and the frames and cases both tests are held to.  An
implementation is a class Sequence(width, height, **SETTINGS) with push_halves(half_a, half_b, features, cam) -> dict of OUTPUTS (every field of
rttnw_svgf_out and of rttnw_svgf_halves) and, for the two on the host, a `state` the caller may read."""
import ctypes as C
import os
import subprocess

import numpy as np

import denoise_ref
import regress_ref
import svgf_cases
import svgf_ref
import temporal_ref
import variance_ref
from rttnw_amd import abi
from temporal_cases import same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALVES = ("acc_a", "acc_b", "filtered_a", "filtered_b", "fit")
OUTPUTS = svgf_ref.OUTPUTS + HALVES
# the handle's settings (svgf_ref.SETTINGS without feedback: the stage is exclusive with it) and the stage's own
SETTINGS = dict({k: v for k, v in svgf_ref.SETTINGS.items() if k != "feedback"}, mask=7, variance_source=0, ridge=0.0, search_radius=0, patch_radius=0, k=0.0)
_LIB = []

# ---- the frames: the smallest sizes at which the kernels can go wrong
SIZES = [(45, 37), (70, 9), (5, 3)]     # ragged against 8x8 trace tiles, 64x4 accumulate blocks and the 16- and 32-pixel filter tiles, one 32-tile
                                        # border crossed on each axis; a 64-wide block border crossed; smaller than every window
SMALL_RADII = dict(search_radius=2, patch_radius=1)
# (size, demodulate, mask, variance_source, a NaN in half_a of the second frame, the filter's default radii)
CASES = [(size, dm, mask, src, False, False) for size in SIZES for dm in (0, 1) for mask in (0, 7) for src in (0, 1)]
CASES += [(SIZES[0], 1, mask, src, True, False) for mask in (0, 7) for src in (0, 1)] + [(SIZES[1], 0, 7, 0, True, False)]
CASES += [(SIZES[0], 1, 7, 0, False, True)]
CASE_IDS = ["%dx%d-%s-%s-%s%s%s" % (s[0], s[1], "albedo" if dm else "colour", "regress" if mask else "nlm", "pair" if src else "temporal",
                                    "-nan" if nan else "", "-default-radii" if big else "") for s, dm, mask, src, nan, big in CASES]


def settings(case):
    (_, dm, mask, src, _, big) = case
    return dict(demodulate=bool(dm), mask=mask, variance_source=src, min_temporal=2, radius=2, iterations=3, **({} if big else SMALL_RADII))


def frames(case):
    """[(half_a, half_b, features, cam)] * 3: a plane seen from 9 units, the camera moved sideways by 0.4 pixels a frame (svgf_cases.moved); a
    textured albedo with channels under the demodulation threshold, a depth ramp, normals that lean, fractional alphas and a region of alpha == 0;
    two noisy halves of a shaded colour per frame."""
    (w, h) = case[0]
    rng = np.random.default_rng(1000 * w + 10 * h + case[1] + 2 * case[2] + 4 * case[3])
    yy, xx = np.mgrid[0:h, 0:w]
    albedo = 0.2 + 0.8 * rng.random((h, w, 3))
    albedo[rng.random((h, w)) < 0.05, 1] = 5e-4
    normal = np.stack([0.15 * np.sin(0.3 * xx), 0.1 * np.cos(0.4 * yy), np.ones((h, w))], axis=-1)
    normal /= np.linalg.norm(normal, axis=-1, keepdims=True)
    alpha = np.ones((h, w))
    alpha[rng.random((h, w)) < 0.1] = 0.5
    alpha[:max(h // 4, 1), w - max(w // 5, 1):] = 0.0                  # the sky: a region of alpha == 0
    alpha[(xx + 3 * yy) % 17 == 5] = 0.0
    z = 9.0 * (1.0 + 0.002 * xx)
    f = {"albedo": albedo, "normal": normal, "depth": z * alpha, "alpha": alpha}
    cam0 = svgf_cases.plane_camera(w / h)
    shade = (0.3 + 0.7 * (xx / max(w - 1, 1)))[..., None] * albedo
    out = []
    for k in range(3):
        a = shade * (0.5 + rng.random((h, w, 3)))
        b = shade * (0.5 + rng.random((h, w, 3)))
        if case[4] and k == 1:
            a[h // 2, w // 2, 1] = np.nan
        out.append((a, b, f, svgf_cases.moved(cam0, 0.4 * k, w)))
    return out


def assert_same_outputs(got, want, what=(), names=OUTPUTS):
    for name in names:
        assert same(got[name], want[name]), (name,) + tuple(what)


def check_chain(make, reference, case):
    """Every field of rttnw_svgf_out and of rttnw_svgf_halves of every link equals `reference`'s bit for bit, both chains on their own state."""
    (w, h) = case[0]
    kw = settings(case)
    got, want = make(w, h, **kw), reference(w, h, **kw)
    for k, (a, b, f, cam) in enumerate(frames(case)):
        x, y = got.push_halves(a, b, f, cam), want.push_halves(a, b, f, cam)
        assert_same_outputs(x, y, (k,))
        if k > 0 and min(w, h) > 4:
            assert (y["length"] == k + 1.0).mean() > 0.3, k                                  # the history was found: the taps carried the halves
    for closing in (got, want):
        if hasattr(closing, "close"):
            closing.close()


def _settings(kw):
    unknown = set(kw) - set(SETTINGS)
    assert not unknown, unknown
    return dict(SETTINGS, **kw)


class Restated:
    """The composition, step by step as the header numbers them."""

    def __init__(self, width, height, **kw):
        self.width, self.height, self.s, self.state = width, height, _settings(kw), None

    def push_halves(self, half_a, half_b, features, cam):
        s, st = self.s, self.state
        a, b = np.ascontiguousarray(half_a, dtype=np.float64), np.ascontiguousarray(half_b, dtype=np.float64)
        F = {k: np.ascontiguousarray(features[k], dtype=np.float64) for k in ("albedo", "normal", "depth", "alpha")}
        assert a.shape == b.shape == (self.height, self.width, 3)
        C_ = (a + b) * 0.5
        # 0
        divided = np.zeros(C_.shape, dtype=bool)
        c, ca, cb = C_, a, b
        if s["demodulate"]:
            divided = (F["alpha"][..., None] != 0.0) & (F["albedo"] > svgf_ref.ALBEDO_EPS)
            with np.errstate(all="ignore"):
                c, ca, cb = (np.where(divided, x / F["albedo"], x) for x in (C_, a, b))
        # 1
        t = dict(max_history=s["max_history"], depth_tolerance=s["depth_tolerance"], normal_min=s["normal_min"])
        history = None if st is None else {"linear": st["M1"], "moment2": st["M2"], "length": st["L"], "features": st["features"], "cam": st["cam"]}
        TV = variance_ref.estimate(c, F, cam, history=history, min_temporal=s["min_temporal"], radius=s["radius"], sigma_normal=s["variance_sigma_normal"],
                                   sigma_depth=s["variance_sigma_depth"], **t)
        # 2
        Aa, Ab = ca, cb
        if st is not None:
            over = [temporal_ref.accumulate(x, F, cam, history={"linear": st[H], "variance": None, "length": st["L"], "features": st["features"],
                                                                "cam": st["cam"]}, **t) for x, H in ((ca, "Ha"), (cb, "Hb"))]
            for o in over:
                assert np.array_equal(o["length"], TV["length"]) and np.array_equal(o["prev_xy"], TV["prev_xy"], equal_nan=True)
            Aa, Ab = over[0]["linear"], over[1]["linear"]
        # 3
        var = TV["variance"]
        half_var = var + var if s["variance_source"] == 0 else None
        R = regress_ref.denoise_regress(Aa, Ab, half_var, half_var, F, mask=s["mask"], demodulate=False, ridge=s["ridge"], search_radius=s["search_radius"],
                                        patch_radius=s["patch_radius"], k=s["k"])
        # 5
        with np.errstate(all="ignore"):
            shown = np.where(divided, R["linear"] * F["albedo"], R["linear"])
            mean = (Aa + Ab) * 0.5
            accumulated = np.where(divided, mean * F["albedo"], mean)
        out = {"linear_rgb": shown, "rgba8": denoise_ref.quantise(shown), "accumulated_rgb": accumulated, "variance_rgb": var,
               "filtered_variance_rgb": R["error"], "length": TV["length"], "prev_xy": TV["prev_xy"], "moment1_rgb": TV["linear"],
               "moment2_rgb": TV["moment2"], "history_rgb": TV["linear"], "raw_rgb": C_, "albedo": F["albedo"], "normal": F["normal"], "depth": F["depth"],
               "alpha": F["alpha"], "acc_a": Aa, "acc_b": Ab, "filtered_a": R["half_a"], "filtered_b": R["half_b"], "fit": R["fit"]}
        self.state = {"M1": TV["linear"], "M2": TV["moment2"], "Ha": Aa, "Hb": Ab, "L": TV["length"], "features": F, "cam": cam}
        return out


def params_of(s):
    """(rttnw_svgf_params, rttnw_regress_params, variance_source) of a dict of SETTINGS."""
    q = svgf_ref.params_of(dict({k: s[k] for k in svgf_ref.SETTINGS if k != "feedback"}, feedback=0))
    g = abi.Regress(search_radius=s["search_radius"], patch_radius=s["patch_radius"], k=s["k"], ridge=s["ridge"], features=s["mask"], demodulate=0,
                    reserved0=0, reserved1=0)
    return q, g, int(s["variance_source"])


def empty_outputs(h, w):
    out = svgf_ref.empty_outputs(h, w)
    out.update({name: np.zeros((h, w) if name == "fit" else (h, w, 3)) for name in HALVES})
    return out


def _lib():
    if not _LIB:
        subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "svgf_regress_host"), "-s"], check=True)
        lib = C.CDLL(os.path.join(ROOT, "tests", "svgf_regress_host", "libsvgf_regress_host.so"))
        lib.srh_svgf_push_halves.argtypes = ([C.c_uint32, C.c_uint32, C.POINTER(abi.Svgf), C.POINTER(abi.Regress), C.c_uint32] + [C.c_void_p] * 16 +
                                             [C.POINTER(abi.SvgfOut)] + [C.c_void_p] * 5)
        lib.srh_svgf_push_halves.restype = C.c_int
        _LIB.append(lib)
    return _LIB[0]


class Host:
    """srh_svgf_push_halves of tests/svgf_regress_host, with the state kept here between the calls."""

    def __init__(self, width, height, **kw):
        self.width, self.height, self.s, self.state, self.lib = width, height, _settings(kw), None, _lib()

    def push_halves(self, half_a, half_b, features, cam):
        st, h, w = self.state, self.height, self.width
        a, b = np.ascontiguousarray(half_a, dtype=np.float64), np.ascontiguousarray(half_b, dtype=np.float64)
        f = [np.ascontiguousarray(features[k], dtype=np.float64) for k in ("albedo", "normal", "depth", "alpha")]
        prev = [None] * 8
        if st is not None:
            pf = st["features"]
            prev = [np.ascontiguousarray(x, dtype=np.float64) for x in (st["M1"], st["M2"], st["Ha"], st["Hb"], st["L"], pf["normal"], pf["depth"], pf["alpha"])]
        arrays = empty_outputs(h, w)
        out = abi.SvgfOut(image_ms=None, **{name: arrays[name].ctypes.data for name in svgf_ref.OUTPUTS})
        q, g, source = params_of(self.s)
        ptr = lambda x: None if x is None else x.ctypes.data
        rc = self.lib.srh_svgf_push_halves(w, h, C.byref(q), C.byref(g), source, C.addressof(cam), None if st is None else C.addressof(st["cam"]), ptr(a), ptr(b),
                                           *[ptr(x) for x in f], *[ptr(x) for x in prev], C.byref(out), *[arrays[name].ctypes.data for name in HALVES])
        assert rc == 0
        self.state = {"M1": arrays["moment1_rgb"], "M2": arrays["moment2_rgb"], "Ha": arrays["acc_a"], "Hb": arrays["acc_b"], "L": arrays["length"],
                      "features": dict(zip(("albedo", "normal", "depth", "alpha"), f)), "cam": cam}
        return arrays
