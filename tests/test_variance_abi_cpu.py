"""rttnw_temporal_variance without a GPU: the export exists and is declared alike in the header, the ctypes binding and the Rust binding;
rttnw_variance_params has one layout in all three; the header states the contract; every argument refusal comes before the device is touched,
in the order the header lists them, with a message that names the entry point and the argument; a valid call without a device fails loudly;
the Python driver and the command line refuse what they must before the library is called.  (tests/test_variance_cpu.py has the arithmetic,
tests/test_gpu_variance.py what the device computes.)"""
import ctypes as C
import re

import numpy as np
import pytest

from abi_cases import FFI, HEADER, HEADER_TEXT, INVALID, RUST_SCENE, camera, cli_refuses, declared_alike, exported
from rttnw_amd import abi, library, render

_D, _U8, _CD = ("double*", "*mut f64", C.c_void_p), ("uint8_t*", "*mut u8", C.c_void_p), ("const double*", "*const f64", C.c_void_p)
_CAM = ("const rttnw_camera_desc*", "*const rttnw_camera_desc", C.POINTER(abi.CameraDesc))
INPUTS = ("linear_rgb", "normal", "depth", "alpha", "prev_linear_rgb", "prev_moment2_rgb", "prev_length", "prev_normal", "prev_depth", "prev_alpha")
ARGS = ([("width", "uint32_t", "u32", C.c_uint32), ("height", "uint32_t", "u32", C.c_uint32), ("cam",) + _CAM, ("prev_cam",) + _CAM] +
        [(name,) + _CD for name in INPUTS] +
        [("t", "const rttnw_temporal_params*", "*const rttnw_temporal_params", C.POINTER(abi.Temporal)),
         ("v", "const rttnw_variance_params*", "*const rttnw_variance_params", C.POINTER(abi.Variance)), ("out_linear_rgb",) + _D, ("out_rgba8",) + _U8,
         ("out_moment2_rgb",) + _D, ("out_length",) + _D, ("out_prev_xy",) + _D, ("out_variance_rgb",) + _D,
         ("kernel_ms", "double*", "*mut f64", C.POINTER(C.c_double))])
HIP = -4


def test_export_and_declarations():
    exported("temporal_variance")
    declared_alike("temporal_variance", ARGS)
    assert "rttnw_temporal_variance" in HEADER_TEXT.split("typedef struct rttnw_scene")[0], "the comment at RTTNW_ABI_VERSION says how a caller detects the function"
    assert "pub fn temporal_variance(" in RUST_SCENE, "the crate's safe wrapper"


def test_params_layout_agrees_in_header_ctypes_and_rust():
    body = re.search(r"struct rttnw_variance_params \{(.*?)\};", HEADER, flags=re.S).group(1)
    c_fields = [" ".join(d.split()) for d in body.split(";") if d.strip()]
    assert c_fields == ["uint32_t min_temporal", "uint32_t radius", "double sigma_normal, sigma_depth", "uint32_t reserved0, reserved1"]
    assert re.search(r"typedef struct rttnw_variance_params rttnw_variance_params;", HEADER)
    attrs, rs_body = re.search(r"((?:#\[[^\]]*\]\s*)+)pub struct rttnw_variance_params\s*\{(.*?)\n\}", FFI, flags=re.S).groups()
    assert "repr(C)" in attrs
    fields = [("min_temporal", "u32", C.c_uint32), ("radius", "u32", C.c_uint32), ("sigma_normal", "f64", C.c_double), ("sigma_depth", "f64", C.c_double),
              ("reserved0", "u32", C.c_uint32), ("reserved1", "u32", C.c_uint32)]
    assert re.findall(r"pub (\w+)\s*:\s*(\w+),", rs_body) == [(n, r) for n, r, _ in fields]
    assert list(abi.Variance._fields_) == [(n, t) for n, _, t in fields]
    assert C.sizeof(abi.Variance) == 32 and [getattr(abi.Variance, n).offset for n, _, _ in fields] == [0, 4, 8, 16, 24, 28]


def test_the_header_states_the_contract_the_three_implementations_share():
    contract = HEADER_TEXT.split("struct rttnw_variance_params {")[0].split("int rttnw_temporal_accumulate(", 1)[1]
    contract = re.sub(r"\n \*\s*", " ", contract)                       # the comment's line breaks are not part of its wording
    for phrase in ("Schied et al. 2017, section 4.2", "no CPU fallback", "prev_moment2_rgb among them", "bit-identical to that entry point's",
                   "h2 = (sum wt * m2') / W", "s = cur * cur (rounded once)", "out_m2 = (1 - a) * h2 + a * s", "two products and one sum, not fused",
                   "out_m2 = s in every case in which the colour passes through", "pos(x) = x < 0 ? 0 : x", "a NaN stays a NaN",
                   "alpha == 0: var = 0", "N >= min_temporal: var = pos(m2 - m1 * m1) / (N - 1)", "dy = -radius .. radius (outer)",
                   "w = w_n * w_z", "w_n = (n0 * n'0 + n1 * n'1) + n2 * n'2", "squared k times",
                   "qz = (z - z') / ((sigma_depth * (abs(z) + abs(z'))) * 0.5 + 1e-12)", "r = 1 / (1 + qz * qz)", "w_z = r * r",
                   "no B-spline factor and no colour stop", "M1 = (sum w * m1') / Sw", "M2 = (sum w * m2') / Sw", "var = pos(M2 - M1 * M1) / N",
                   "Sw > 0 false: var = pos(m2 - m1 * m1) / N", "Every sum starts from 0.0", "give the same bits", "can be handed to it as variance_rgb",
                   "device time of both kernels", "Out of scope", "albedo-demodulated moments", "luminance-only moments",
                   "a device-resident chain between frames", "feeding the filtered image back", "a node-wide form", "the native rttnw program"):
        assert phrase in contract, phrase


def _call(b, drop=(), width=4, height=3, t=None, **vkw):
    n = max(width * height, 1) * 3
    arr = {k: np.ones(n) for k in INPUTS}
    tp = abi.Temporal(max_history=0, reserved0=0, depth_tolerance=0.0, normal_min=0.0)
    for key, val in (t or {}).items():
        setattr(tp, key, val)
    vp = abi.Variance(min_temporal=0, radius=0, sigma_normal=0.0, sigma_depth=0.0, reserved0=0, reserved1=0)
    for key, val in vkw.items():
        setattr(vp, key, val)
    cam, prev_cam = camera(), camera()
    ptr = lambda k: None if k in drop else arr[k].ctypes.data
    return b.temporal_variance(width, height, None if "cam" in drop else C.byref(cam), None if "prev_cam" in drop else C.byref(prev_cam),
                               *[ptr(k) for k in INPUTS], None if "t" in drop else C.byref(tp), None if "v" in drop else C.byref(vp),
                               None, None, None, None, None, None, None)


PREV = ("prev_linear_rgb", "prev_moment2_rgb", "prev_length", "prev_normal", "prev_depth", "prev_alpha")
# in the order the entry point checks: each refusal is reached with everything before it in order
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
    ("only prev_moment2_rgb", {"drop": tuple(k for k in PREV if k != "prev_moment2_rgb")}, "prev_* arrays go together"),
    ("only prev_alpha", {"drop": PREV[:5]}, "prev_* arrays go together"),
    ("a history without prev_cam", {"drop": ("prev_cam",)}, "prev_cam is NULL"),
    ("max_history 65536", {"t": {"max_history": 65536}}, "t->max_history"),
    ("t's reserved0", {"t": {"reserved0": 1}}, "t->reserved0"),
    ("negative depth_tolerance", {"t": {"depth_tolerance": -0.1}}, "t->depth_tolerance"),
    ("NaN depth_tolerance", {"t": {"depth_tolerance": float("nan")}}, "t->depth_tolerance"),
    ("normal_min 1.5", {"t": {"normal_min": 1.5}}, "t->normal_min"),
    ("NaN normal_min", {"t": {"normal_min": float("nan")}}, "t->normal_min"),
    ("NULL v", {"drop": ("v",)}, "v is NULL"),
    ("min_temporal 1", {"min_temporal": 1}, "v->min_temporal"),
    ("min_temporal 65536", {"min_temporal": 65536}, "v->min_temporal"),
    ("radius 5", {"radius": 5}, "v->radius"),
    ("reserved0", {"reserved0": 1}, "v->reserved0"),
    ("reserved1", {"reserved1": 7}, "v->reserved1"),
    ("negative sigma_normal", {"sigma_normal": -1.0}, "v->sigma_normal"),
    ("NaN sigma_normal", {"sigma_normal": float("nan")}, "v->sigma_normal"),
    ("negative sigma_depth", {"sigma_depth": -0.5}, "v->sigma_depth"),
    ("NaN sigma_depth", {"sigma_depth": float("nan")}, "v->sigma_depth"),
]


@pytest.mark.parametrize("what,kw,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_come_before_the_device(what, kw, msg):
    b = library.product()
    assert _call(b, **kw) == INVALID, what
    err = b.last_error().decode()
    assert err.startswith("temporal_variance:") and msg in err, (what, err)


def test_an_earlier_refusal_wins():
    """The order of the header's list: the shared arguments, the history, t's fields, then v and its fields."""
    b = library.product()
    for first, then in (({"drop": ("cam", "v")}, "cam is NULL"), ({"drop": ("prev_alpha", "v")}, "prev_* arrays"),
                        ({"t": {"max_history": 65536}, "drop": ("v",)}, "t->max_history"), ({"min_temporal": 1, "radius": 9}, "v->min_temporal"),
                        ({"radius": 9, "reserved0": 1}, "v->radius"), ({"reserved1": 1, "sigma_depth": -1.0}, "v->reserved0")):
        assert _call(b, **first) == INVALID
        assert then in b.last_error().decode(), (first, b.last_error().decode())


@pytest.mark.skipif(library.product().device_count() > 0, reason="a GPU is present")
@pytest.mark.parametrize("kw", [{}, {"drop": PREV + ("prev_cam",)}, {"drop": PREV}, {"min_temporal": 2, "radius": 4, "sigma_normal": 1.0, "sigma_depth": 3.0},
                                {"min_temporal": 65535, "radius": 1}, {"t": {"max_history": 65535, "normal_min": -1.0}}])
def test_a_valid_call_without_a_device_fails_loudly(kw):
    b = library.product()
    assert _call(b, **kw) == HIP
    assert "no CPU fallback" in b.last_error().decode() and "temporal_variance" in b.last_error().decode()


def test_the_python_driver_refuses_before_the_library_is_called():
    img, plane = np.zeros((4, 5, 3)), np.zeros((4, 5))
    f = {"albedo": img, "normal": img, "depth": plane, "alpha": plane}
    cam = camera()
    history = {"linear": img, "moment2": img, "length": plane, "features": f, "cam": cam}
    with pytest.raises(ValueError, match="HxWx3"):
        render.temporal_variance(plane, f, cam)
    with pytest.raises(ValueError, match="it lacks moment2"):
        render.temporal_variance(img, f, cam, history=dict(history, moment2=None))
    with pytest.raises(ValueError, match="it lacks moment2, length, cam"):
        render.temporal_variance(img, f, cam, history={"linear": img, "features": f})
    with pytest.raises(ValueError, match="of one 5x4 frame"):
        render.temporal_variance(img, f, cam, history=dict(history, moment2=np.zeros((4, 6, 3))))
    with pytest.raises(ValueError, match="of one 5x4 frame"):
        render.temporal_variance(img, dict(f, depth=np.zeros((3, 5))), cam)
    for kw, name in (({"max_history": 65536}, "max_history"), ({"depth_tolerance": -1.0}, "depth_tolerance"), ({"normal_min": 1.5}, "normal_min"),
                     ({"min_temporal": 1}, "min_temporal"), ({"min_temporal": 65536}, "min_temporal"), ({"min_temporal": -2}, "min_temporal"),
                     ({"radius": 5}, "radius"), ({"radius": -1}, "radius"), ({"sigma_normal": -1.0}, "sigma_normal"),
                     ({"sigma_depth": float("nan")}, "sigma_depth")):
        with pytest.raises(ValueError, match=name):
            render.temporal_variance(img, f, cam, **kw)
    with pytest.raises(ValueError, match="variance needs temporal"):
        render.render_sequence(None, [], None, temporal=False, variance=True)
    with pytest.raises(ValueError, match="stderr or variance, not both"):
        render.denoise(img, f, stderr=img, variance=img)


@pytest.mark.parametrize("argv,msg", [
    (["7", "--temporal-variance"], "--temporal-variance needs --orbit"),
    (["7", "--orbit", "3", "--temporal-variance", "--noise", "0.1"], "--orbit does not combine with --noise"),
    (["7", "--orbit", "3", "--temporal-variance", "--denoise-select"], "--orbit does not combine with --denoise-select"),
    (["7", "--orbit", "0", "--temporal-variance"], "--orbit must be 1 .. 1000"),
])
def test_cli_refuses_before_any_scene_is_built(argv, msg, tmp_path):
    cli_refuses(argv, msg, tmp_path, must_not_exist=("frame_000.png",))
