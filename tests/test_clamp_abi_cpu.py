"""rttnw_temporal_clamp, rttnw_svgf_set_clamp and rttnw_svgf_clipped without a GPU: the exports exist and are declared alike in the header, the
ctypes binding and the Rust binding; rttnw_clamp_params has one layout in all three; the header states the contract and leaves its neighbours'
blocks alone; every argument refusal comes before the device is touched, in the order the header lists them, with a message that names the entry
point and the argument; a valid call without a device fails loudly; the Python driver and the command line refuse what they must before the
library is called.  (tests/test_clamp_cpu.py has the arithmetic, tests/test_gpu_clamp.py what the device computes.)"""
import ctypes as C
import re

import numpy as np
import pytest

from abi_cases import FFI, HEADER, HEADER_TEXT, INVALID, camera, cli_refuses, declared_alike, exported
from rttnw_amd import abi, library, render

_D, _U8, _CD = ("double*", "*mut f64", C.c_void_p), ("uint8_t*", "*mut u8", C.c_void_p), ("const double*", "*const f64", C.c_void_p)
_CAM = ("const rttnw_camera_desc*", "*const rttnw_camera_desc", C.POINTER(abi.CameraDesc))
_Q = ("rttnw_svgf*", "*mut rttnw_svgf", C.c_void_p)
_K = ("const rttnw_clamp_params*", "*const rttnw_clamp_params", C.POINTER(abi.Clamp))
INPUTS = ("linear_rgb", "normal", "depth", "alpha", "prev_linear_rgb", "prev_moment2_rgb", "prev_length", "prev_normal", "prev_depth", "prev_alpha")
ARGS = ([("width", "uint32_t", "u32", C.c_uint32), ("height", "uint32_t", "u32", C.c_uint32), ("cam",) + _CAM, ("prev_cam",) + _CAM] +
        [(name,) + _CD for name in INPUTS] +
        [("t", "const rttnw_temporal_params*", "*const rttnw_temporal_params", C.POINTER(abi.Temporal)),
         ("v", "const rttnw_variance_params*", "*const rttnw_variance_params", C.POINTER(abi.Variance)), ("k",) + _K, ("out_linear_rgb",) + _D,
         ("out_rgba8",) + _U8, ("out_moment2_rgb",) + _D, ("out_length",) + _D, ("out_prev_xy",) + _D, ("out_variance_rgb",) + _D,
         ("out_mean_rgb",) + _D, ("out_sd_rgb",) + _D, ("out_clipped",) + _U8, ("kernel_ms", "double*", "*mut f64", C.POINTER(C.c_double))])
HIP = -4
NAN, INF = float("nan"), float("inf")


def test_exports_and_declarations():
    for name in ("temporal_clamp", "svgf_set_clamp", "svgf_clipped"):
        exported(name)
        assert "rttnw_" + name in HEADER_TEXT.split("typedef struct rttnw_scene")[0], "the comment at RTTNW_ABI_VERSION says how a caller detects the function"
    declared_alike("temporal_clamp", ARGS)
    declared_alike("svgf_set_clamp", [("q",) + _Q, ("k",) + _K])
    declared_alike("svgf_clipped", [("q",) + _Q, ("out_clipped",) + _U8])


def test_the_entry_point_takes_temporal_variances_arguments_in_their_order():
    def names(fn):
        proto = re.search(r"\bint rttnw_%s\((.*?)\);" % fn, HEADER, flags=re.S).group(1)
        return [re.match(r".+?(\w+)$", a.strip()).group(1) for a in " ".join(proto.split()).split(",")]
    theirs, ours = names("temporal_variance"), names("temporal_clamp")
    at = theirs.index("v") + 1
    assert ours[:at] == theirs[:at] and ours[at] == "k"
    assert ours[at + 1:] == theirs[at:-1] + ["out_mean_rgb", "out_sd_rgb", "out_clipped", "kernel_ms"]
    assert HEADER.index("int rttnw_temporal_clamp(") > HEADER.index("int rttnw_svgf_frame("), "the new block stands after rttnw_svgf_frame"


def test_params_layout_agrees_in_header_ctypes_and_rust():
    body = re.search(r"struct rttnw_clamp_params \{(.*?)\};", HEADER, flags=re.S).group(1)
    c_fields = [" ".join(d.split()) for d in body.split(";") if d.strip()]
    assert c_fields == ["uint32_t radius", "uint32_t reserved0", "double gamma", "double sigma_normal, sigma_depth"]
    assert re.search(r"typedef struct rttnw_clamp_params rttnw_clamp_params;", HEADER)
    attrs, rs_body = re.search(r"((?:#\[[^\]]*\]\s*)+)pub struct rttnw_clamp_params\s*\{(.*?)\n\}", FFI, flags=re.S).groups()
    assert "repr(C)" in attrs
    fields = [("radius", "u32", C.c_uint32), ("reserved0", "u32", C.c_uint32), ("gamma", "f64", C.c_double), ("sigma_normal", "f64", C.c_double),
              ("sigma_depth", "f64", C.c_double)]
    assert re.findall(r"pub (\w+)\s*:\s*(\w+),", rs_body) == [(n, r) for n, r, _ in fields]
    assert list(abi.Clamp._fields_) == [(n, t) for n, _, t in fields]
    assert C.sizeof(abi.Clamp) == 32 and [getattr(abi.Clamp, n).offset for n, _, _ in fields] == [0, 4, 8, 16, 24]
    assert C.sizeof(abi.Svgf) == 104 and C.sizeof(abi.SvgfOut) == 8 * 16, "the handle's two blocks keep their layout"


def test_the_header_states_the_contract():
    contract = HEADER_TEXT.split("struct rttnw_clamp_params {")[0].split("int rttnw_svgf_frame(", 1)[1]
    contract = re.sub(r"\n \*\s*", " ", contract)                       # the comment's line breaks are not part of its wording
    for phrase in ("Karis 2014", "Salvi 2016", "clipping now lives here", "no CPU fallback", "k after v", "three optional outputs before kernel_ms",
                   "dy = -radius .. radius (outer)", "whose alpha == 0, are dropped", "w = w_n * w_z", "with radius and sigmas from k",
                   "m1' = cur", "m2' = cur * cur (rounded once)", "mu = (sum w * m1') / Sw", "q = (sum w * m2') / Sw", "otherwise mu = cur and q = cur * cur",
                   "sd = sqrt(pos(q - mu * mu))", "A pixel with alpha == 0 has mu = cur, sd = 0", "lo = mu - gamma * sd", "hi = mu + gamma * sd",
                   "one product and one sum each, not fused", "out_mean_rgb = mu and out_sd_rgb = sd, for every pixel",
                   "h1 = (sum wt * m1') / W", "h2 = (sum wt * m2') / W", "h1c = h1 < lo ? lo : (h1 > hi ? hi : h1)",
                   "Every comparison with a NaN is false", "the inf * 0 bounds of gamma = +inf with sd = 0 clip nothing",
                   "Bit ch of out_clipped is set exactly where one of the two branches was taken", "h2c = (h2 - h1 * h1) + h1c * h1c",
                   "keeps its spread about the moved mean", "a branch, not arithmetic", "with out_clipped = 0", "rttnw_temporal_variance's, unchanged",
                   "Where no channel of a pixel is clipped, every shared output equals rttnw_temporal_variance's bits",
                   "With gamma = +inf every shared output equals rttnw_temporal_variance's bits and out_clipped is all 0", "give the same bits",
                   "naming temporal_clamp", "a NULL k, k->radius > 4, k->reserved0 != 0, a negative or NaN gamma, a negative or NaN sigma",
                   "takes effect from the next frame call", "keeps the history", "the handle is checked last", "frame calls still allocate nothing",
                   "TV = rttnw_temporal_clamp(", "prev_linear_rgb = H, prev_moment2_rgb = M2, prev_length = L",
                   "H is clipped to the same interval as M1", "bits 0 - 2 are TV's out_clipped, bits 4 - 6 the H call's (0 without feedback)",
                   "before any frame call, or after a call without a clamp, the map is all 0", "a texture does not widen the interval",
                   "every field of rttnw_svgf_out equals the unclamped handle's bits", "Out of scope", "another colour space (YCoCg)",
                   "cutting the history length where a pixel was clipped", "a \"fast history\"", "a node-wide form", "the native rttnw program"):
        assert phrase in contract, phrase


def test_the_neighbours_blocks_still_leave_clamping_out_of_their_scope():
    """The three blocks above the new one are as they were: each names the gap, and the new block says where it went."""
    before = HEADER_TEXT.split("int rttnw_svgf_frame(")[0]
    assert "colour clamping of the history" in before and "colour clamping; a device-resident chain between frames" in re.sub(r"\n \*\s*", " ", before)
    assert re.search(r"#define RTTNW_ABI_VERSION 3\b", HEADER)


def _call(b, drop=(), width=4, height=3, t=None, v=None, **kkw):
    n = max(width * height, 1) * 3
    arr = {name: np.ones(n) for name in INPUTS}
    tp = abi.Temporal(max_history=0, reserved0=0, depth_tolerance=0.0, normal_min=0.0)
    for key, val in (t or {}).items():
        setattr(tp, key, val)
    vp = abi.Variance(min_temporal=0, radius=0, sigma_normal=0.0, sigma_depth=0.0, reserved0=0, reserved1=0)
    for key, val in (v or {}).items():
        setattr(vp, key, val)
    kp = abi.Clamp(radius=0, reserved0=0, gamma=0.0, sigma_normal=0.0, sigma_depth=0.0)
    for key, val in kkw.items():
        setattr(kp, key, val)
    cam, prev_cam = camera(), camera()
    ptr = lambda name: None if name in drop else arr[name].ctypes.data
    return b.temporal_clamp(width, height, None if "cam" in drop else C.byref(cam), None if "prev_cam" in drop else C.byref(prev_cam),
                            *[ptr(name) for name in INPUTS], None if "t" in drop else C.byref(tp), None if "v" in drop else C.byref(vp),
                            None if "k" in drop else C.byref(kp), *([None] * 10))


PREV = ("prev_linear_rgb", "prev_moment2_rgb", "prev_length", "prev_normal", "prev_depth", "prev_alpha")
K_REFUSALS = [
    ("NULL k", {"drop": ("k",)}, "k is NULL"),
    ("radius 5", {"radius": 5}, "k->radius"),
    ("reserved0", {"reserved0": 1}, "k->reserved0"),
    ("negative gamma", {"gamma": -0.5}, "k->gamma"),
    ("-inf gamma", {"gamma": -INF}, "k->gamma"),
    ("NaN gamma", {"gamma": NAN}, "k->gamma"),
    ("negative sigma_normal", {"sigma_normal": -1.0}, "k->sigma_normal"),
    ("NaN sigma_normal", {"sigma_normal": NAN}, "k->sigma_normal"),
    ("negative sigma_depth", {"sigma_depth": -0.5}, "k->sigma_depth"),
    ("NaN sigma_depth", {"sigma_depth": NAN}, "k->sigma_depth"),
]
# in the order the entry point checks: rttnw_temporal_variance's list (tests/test_variance_abi_cpu.py), then k's
REFUSALS = [
    ("NULL cam", {"drop": ("cam",)}, "cam is NULL"),
    ("NULL linear_rgb", {"drop": ("linear_rgb",)}, "linear_rgb"),
    ("NULL normal", {"drop": ("normal",)}, "normal"),
    ("NULL depth", {"drop": ("depth",)}, "depth"),
    ("NULL alpha", {"drop": ("alpha",)}, "alpha"),
    ("NULL t", {"drop": ("t",)}, "t is NULL"),
    ("width 0", {"width": 0}, "width * height"),
    ("height 0", {"height": 0}, "width * height"),
] + [("without " + name, {"drop": (name,)}, "prev_* arrays go together") for name in PREV] + [
    ("only prev_moment2_rgb", {"drop": tuple(name for name in PREV if name != "prev_moment2_rgb")}, "prev_* arrays go together"),
    ("only prev_alpha", {"drop": PREV[:5]}, "prev_* arrays go together"),
    ("a history without prev_cam", {"drop": ("prev_cam",)}, "prev_cam is NULL"),
    ("max_history 65536", {"t": {"max_history": 65536}}, "t->max_history"),
    ("t's reserved0", {"t": {"reserved0": 1}}, "t->reserved0"),
    ("negative depth_tolerance", {"t": {"depth_tolerance": -0.1}}, "t->depth_tolerance"),
    ("NaN depth_tolerance", {"t": {"depth_tolerance": NAN}}, "t->depth_tolerance"),
    ("normal_min 1.5", {"t": {"normal_min": 1.5}}, "t->normal_min"),
    ("NaN normal_min", {"t": {"normal_min": NAN}}, "t->normal_min"),
    ("NULL v", {"drop": ("v",)}, "v is NULL"),
    ("min_temporal 1", {"v": {"min_temporal": 1}}, "v->min_temporal"),
    ("min_temporal 65536", {"v": {"min_temporal": 65536}}, "v->min_temporal"),
    ("v's radius 5", {"v": {"radius": 5}}, "v->radius"),
    ("v's reserved0", {"v": {"reserved0": 1}}, "v->reserved0"),
    ("v's reserved1", {"v": {"reserved1": 7}}, "v->reserved1"),
    ("negative v.sigma_normal", {"v": {"sigma_normal": -1.0}}, "v->sigma_normal"),
    ("NaN v.sigma_depth", {"v": {"sigma_depth": NAN}}, "v->sigma_depth"),
] + K_REFUSALS


@pytest.mark.parametrize("what,kw,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_come_before_the_device(what, kw, msg):
    b = library.product()
    assert _call(b, **kw) == INVALID, what
    err = b.last_error().decode()
    assert err.startswith("temporal_clamp:") and msg in err, (what, err)


def test_an_earlier_refusal_wins():
    """The order of the header's list: rttnw_temporal_variance's, then k and its fields."""
    b = library.product()
    for first, then in (({"drop": ("cam", "k")}, "cam is NULL"), ({"drop": ("prev_alpha", "k")}, "prev_* arrays"),
                        ({"t": {"max_history": 65536}, "drop": ("k",)}, "t->max_history"), ({"v": {"radius": 9}, "radius": 9}, "v->radius"),
                        ({"drop": ("v", "k")}, "v is NULL"), ({"radius": 9, "reserved0": 1}, "k->radius"), ({"reserved0": 1, "gamma": -1.0}, "k->reserved0"),
                        ({"gamma": NAN, "sigma_depth": -1.0}, "k->gamma")):
        assert _call(b, **first) == INVALID
        assert then in b.last_error().decode(), (first, b.last_error().decode())


@pytest.mark.parametrize("what,kw,msg", K_REFUSALS[1:], ids=[r[0] for r in K_REFUSALS[1:]])
def test_set_clamp_refuses_the_same_block_before_it_looks_at_the_handle(what, kw, msg):
    b = library.product()
    kp = abi.Clamp(radius=0, reserved0=0, gamma=0.0, sigma_normal=0.0, sigma_depth=0.0)
    for key, val in kw.items():
        setattr(kp, key, val)
    assert b.svgf_set_clamp(None, C.byref(kp)) == INVALID, what
    err = b.last_error().decode()
    assert err.startswith("svgf_set_clamp:") and msg in err, (what, err)


def test_the_handle_is_checked_last():
    b = library.product()
    for kp in (None, abi.Clamp(), abi.Clamp(radius=4, gamma=INF, sigma_normal=1.0, sigma_depth=3.0)):
        assert b.svgf_set_clamp(None, None if kp is None else C.byref(kp)) == INVALID
        assert b.last_error().decode() == "svgf_set_clamp: q is NULL"
    out = np.zeros(12, dtype=np.uint8)
    assert b.svgf_clipped(None, None) == INVALID and "svgf_clipped: out_clipped is NULL" in b.last_error().decode()
    assert b.svgf_clipped(None, out.ctypes.data) == INVALID and b.last_error().decode() == "svgf_clipped: q is NULL"


@pytest.mark.skipif(library.product().device_count() > 0, reason="a GPU is present")
@pytest.mark.parametrize("kw", [{}, {"drop": PREV + ("prev_cam",)}, {"drop": PREV}, {"radius": 4, "gamma": INF, "sigma_normal": 1.0, "sigma_depth": 3.0},
                                {"radius": 1, "gamma": 0.25}, {"t": {"max_history": 65535, "normal_min": -1.0}, "v": {"min_temporal": 2, "radius": 4}}])
def test_a_valid_call_without_a_device_fails_loudly(kw):
    b = library.product()
    assert _call(b, **kw) == HIP
    assert "no CPU fallback" in b.last_error().decode() and "temporal_clamp" in b.last_error().decode()


def test_the_python_driver_refuses_before_the_library_is_called():
    img, plane = np.zeros((4, 5, 3)), np.zeros((4, 5))
    f = {"albedo": img, "normal": img, "depth": plane, "alpha": plane}
    cam = camera()
    history = {"linear": img, "moment2": img, "length": plane, "features": f, "cam": cam}
    with pytest.raises(ValueError, match="HxWx3"):
        render.temporal_clamp(plane, f, cam)
    with pytest.raises(ValueError, match="it lacks moment2"):
        render.temporal_clamp(img, f, cam, history=dict(history, moment2=None))
    with pytest.raises(ValueError, match="of one 5x4 frame"):
        render.temporal_clamp(img, f, cam, history=dict(history, moment2=np.zeros((4, 6, 3))))
    for kw, name in (({"max_history": 65536}, "max_history"), ({"min_temporal": 1}, "min_temporal"), ({"radius": 5}, "radius"),
                     ({"sigma_depth": NAN}, "sigma_depth"), ({"gamma": -1.0}, "gamma"), ({"gamma": NAN}, "gamma"), ({"clamp_radius": 5}, "clamp_radius"),
                     ({"clamp_radius": -1}, "clamp_radius"), ({"clamp_sigma_normal": -1.0}, "clamp_sigma_normal"), ({"clamp_sigma_depth": NAN}, "clamp_sigma_depth")):
        with pytest.raises(ValueError, match=name):
            render.temporal_clamp(img, f, cam, **kw)
    with pytest.raises(ValueError, match="clamp needs variance"):
        render.render_sequence(None, [], None, clamp=1.0)
    with pytest.raises(ValueError, match="at least 0"):
        render.render_sequence(None, [], None, variance=True, clamp=-1.0)
    with pytest.raises(ValueError, match="at least 0"):
        render.render_sequence_device(None, [], None, clamp=NAN)
    assert set(render.CLAMP_OUTPUTS) == set(render.VARIANCE_OUTPUTS) | {"mean", "sd", "clipped"}


@pytest.mark.parametrize("argv,msg", [
    (["7", "--clamp", "1"], "--clamp needs --temporal-variance or --svgf"),
    (["7", "--orbit", "3", "--clamp", "1"], "--clamp needs --temporal-variance or --svgf"),
    (["7", "--orbit", "3", "--temporal", "--clamp", "1"], "--clamp needs --temporal-variance or --svgf"),
    (["7", "--orbit", "3", "--svgf", "--clamp", "-1"], "--clamp must be at least 0"),
    (["7", "--orbit", "3", "--temporal-variance", "--clamp", "nan"], "--clamp must be at least 0"),
    (["7", "--svgf", "--clamp", "1"], "--svgf needs --orbit"),
])
def test_cli_refuses_before_any_scene_is_built(argv, msg, tmp_path):
    cli_refuses(argv, msg, tmp_path, must_not_exist=("frame_000.png",))
