"""rttnw_temporal_accumulate without a GPU: the export exists and is declared alike in the header, the ctypes binding and the Rust binding;
rttnw_temporal_params has one layout in all three; the header states the contract; every argument refusal comes before the device is touched,
with a message that names the entry point and the argument; a valid call without a device fails loudly; the Python driver and the command line
refuse what they must before the library is called.  (tests/test_temporal_cpu.py has the arithmetic, tests/test_gpu_temporal.py what the device
computes.)"""
import ctypes as C
import re

import numpy as np
import pytest

from abi_cases import FFI, HEADER, HEADER_TEXT, INVALID, RUST_SCENE, camera, cli_refuses, declared_alike, exported
from rttnw_amd import abi, library, render

_D, _U8, _CD = ("double*", "*mut f64", C.c_void_p), ("uint8_t*", "*mut u8", C.c_void_p), ("const double*", "*const f64", C.c_void_p)
_CAM = ("const rttnw_camera_desc*", "*const rttnw_camera_desc", C.POINTER(abi.CameraDesc))
INPUTS = ("linear_rgb", "variance_rgb", "normal", "depth", "alpha", "prev_linear_rgb", "prev_variance_rgb", "prev_length", "prev_normal", "prev_depth",
          "prev_alpha")
ARGS = ([("width", "uint32_t", "u32", C.c_uint32), ("height", "uint32_t", "u32", C.c_uint32), ("cam",) + _CAM, ("prev_cam",) + _CAM] +
        [(name,) + _CD for name in INPUTS] +
        [("t", "const rttnw_temporal_params*", "*const rttnw_temporal_params", C.POINTER(abi.Temporal)), ("out_linear_rgb",) + _D, ("out_rgba8",) + _U8,
         ("out_variance_rgb",) + _D, ("out_length",) + _D, ("out_prev_xy",) + _D, ("kernel_ms", "double*", "*mut f64", C.POINTER(C.c_double))])
HIP = -4


def test_export_and_declarations():
    exported("temporal_accumulate")
    declared_alike("temporal_accumulate", ARGS)
    assert "rttnw_temporal_accumulate" in HEADER_TEXT.split("typedef struct rttnw_scene")[0], "the comment at RTTNW_ABI_VERSION says how a caller detects the function"
    assert "pub fn temporal_accumulate(" in RUST_SCENE, "the crate's safe wrapper"


def test_params_layout_agrees_in_header_ctypes_and_rust():
    body = re.search(r"struct rttnw_temporal_params \{(.*?)\};", HEADER, flags=re.S).group(1)
    c_fields = [" ".join(d.split()) for d in body.split(";") if d.strip()]
    assert c_fields == ["uint32_t max_history", "uint32_t reserved0", "double depth_tolerance", "double normal_min"]
    assert re.search(r"typedef struct rttnw_temporal_params rttnw_temporal_params;", HEADER)
    attrs, rs_body = re.search(r"((?:#\[[^\]]*\]\s*)+)pub struct rttnw_temporal_params\s*\{(.*?)\n\}", FFI, flags=re.S).groups()
    assert "repr(C)" in attrs
    fields = [("max_history", "u32", C.c_uint32), ("reserved0", "u32", C.c_uint32), ("depth_tolerance", "f64", C.c_double), ("normal_min", "f64", C.c_double)]
    assert re.findall(r"pub (\w+)\s*:\s*(\w+),", rs_body) == [(n, r) for n, r, _ in fields]
    assert list(abi.Temporal._fields_) == [(n, t) for n, _, t in fields]
    assert C.sizeof(abi.Temporal) == 24 and [getattr(abi.Temporal, n).offset for n, _, _ in fields] == [0, 4, 8, 16]


def test_the_header_states_the_contract_the_three_implementations_share():
    contract = HEADER_TEXT.split("struct rttnw_temporal_params {")[0].split("int rttnw_denoise_select(", 1)[1]
    contract = re.sub(r"\n \*\s*", " ", contract)                       # the comment's line breaks are not part of its wording
    for phrase in ("Camera::new, camera.rs:32-61", "an aperture above 0 is ignored", "Shutter times are not read", "(a0 * b0 + a1 * b1) + a2 * b2",
                   "s = (x + 0.5) / w", "t = ((h - 1 - y) + 0.5) / h", "d = ((llc + s * H) + t * V) - o", "z = depth / alpha",
                   "P = o + d * (z / sqrt(dot(d, d)))", "lambda = dot(e, n) / dot(q, n)", "r = lambda * q - e", "fx = s' * w - 0.5",
                   "fy = (h - t' * h) - 0.5", "zq = sqrt(dot(q, q))", "lambda > 0 is false", "motion-vector map", "bitwise equal",
                   "fx = x, fy = y, zq = z exactly", "00, 10, 01, 11", "abs(prev_depth / prev_alpha - zq) <= depth_tolerance * zq",
                   "normal_min * sqrt(dot(n, n) * dot(n', n'))", "With normal_min == -1 the normal test is not made", "W > 0 false",
                   "N = min(L + 1, double(max_history))", "a = 1.0 / N", "two products and one sum, not fused",
                   "((1 - a) * (1 - a)) * vh + (a * a) * var", "the plain weighted mean", "they propagate through the sums they enter",
                   "main.rs:219-225, alpha 255", "written only when variance_rgb was given", "give the same bits", "no CPU fallback", "Out of scope",
                   "will ghost", "a device-resident chain between frames"):
        assert phrase in contract, phrase


def _call(b, drop=(), width=4, height=3, **tkw):
    n = max(width * height, 1) * 3
    arr = {k: np.ones(n) for k in INPUTS}
    t = abi.Temporal(max_history=0, reserved0=0, depth_tolerance=0.0, normal_min=0.0)
    for key, v in tkw.items():
        setattr(t, key, v)
    cam, prev_cam = camera(), camera()
    ptr = lambda k: None if k in drop else arr[k].ctypes.data
    return b.temporal_accumulate(width, height, None if "cam" in drop else C.byref(cam), None if "prev_cam" in drop else C.byref(prev_cam),
                                 *[ptr(k) for k in INPUTS], None if "t" in drop else C.byref(t), None, None, None, None, None, None)


PREV = ("prev_linear_rgb", "prev_length", "prev_normal", "prev_depth", "prev_alpha")


@pytest.mark.parametrize("what,kw,msg", [
    ("NULL cam", {"drop": ("cam",)}, "cam is NULL"),
    ("NULL linear_rgb", {"drop": ("linear_rgb",)}, "linear_rgb"),
    ("NULL normal", {"drop": ("normal",)}, "normal"),
    ("NULL depth", {"drop": ("depth",)}, "depth"),
    ("NULL alpha", {"drop": ("alpha",)}, "alpha"),
    ("NULL t", {"drop": ("t",)}, "t is NULL"),
    ("width 0", {"width": 0}, "width * height"),
    ("height 0", {"height": 0}, "width * height"),
] + [("without " + name, {"drop": (name,)}, "prev_* arrays go together") for name in PREV] + [
    ("only prev_variance_rgb", {"drop": PREV}, "prev_* arrays go together"),
    ("only prev_alpha", {"drop": PREV[:4] + ("prev_variance_rgb",)}, "prev_* arrays go together"),
    ("a history without prev_cam", {"drop": ("prev_cam",)}, "prev_cam is NULL"),
    ("variance_rgb alone", {"drop": ("prev_variance_rgb",)}, "variance_rgb and prev_variance_rgb"),
    ("prev_variance_rgb alone", {"drop": ("variance_rgb",)}, "variance_rgb and prev_variance_rgb"),
    ("max_history 65536", {"max_history": 65536}, "t->max_history"),
    ("reserved0", {"reserved0": 1}, "t->reserved0"),
    ("negative depth_tolerance", {"depth_tolerance": -0.1}, "t->depth_tolerance"),
    ("NaN depth_tolerance", {"depth_tolerance": float("nan")}, "t->depth_tolerance"),
    ("normal_min 1.5", {"normal_min": 1.5}, "t->normal_min"),
    ("normal_min -1.5", {"normal_min": -1.5}, "t->normal_min"),
    ("NaN normal_min", {"normal_min": float("nan")}, "t->normal_min"),
])
def test_refusals_come_before_the_device(what, kw, msg):
    b = library.product()
    assert _call(b, **kw) == INVALID, what
    err = b.last_error().decode()
    assert err.startswith("temporal_accumulate:") and msg in err, (what, err)


@pytest.mark.skipif(library.product().device_count() > 0, reason="a GPU is present")
@pytest.mark.parametrize("kw", [{}, {"drop": ("variance_rgb", "prev_variance_rgb")}, {"drop": PREV + ("prev_variance_rgb", "prev_cam")},
                                {"drop": PREV + ("prev_variance_rgb", "prev_cam", "variance_rgb")},
                                {"max_history": 65535, "depth_tolerance": 3.0, "normal_min": -1.0}, {"max_history": 1, "normal_min": 1.0}])
def test_a_valid_call_without_a_device_fails_loudly(kw):
    b = library.product()
    assert _call(b, **kw) == HIP
    assert "no CPU fallback" in b.last_error().decode() and "temporal_accumulate" in b.last_error().decode()


def test_the_python_driver_refuses_before_the_library_is_called():
    img, plane = np.zeros((4, 5, 3)), np.zeros((4, 5))
    f = {"albedo": img, "normal": img, "depth": plane, "alpha": plane}
    cam = camera()
    history = {"linear": img, "variance": None, "length": plane, "features": f, "cam": cam}
    with pytest.raises(ValueError, match="HxWx3"):
        render.temporal_accumulate(plane, f, cam)
    with pytest.raises(ValueError, match="both frames have a variance or neither"):
        render.temporal_accumulate(img, f, cam, history=history, variance=img)
    with pytest.raises(ValueError, match="both frames have a variance or neither"):
        render.temporal_accumulate(img, f, cam, history=dict(history, variance=img))
    with pytest.raises(ValueError, match="it lacks length, cam"):
        render.temporal_accumulate(img, f, cam, history={"linear": img, "features": f})
    with pytest.raises(ValueError, match="of one 5x4 frame"):
        render.temporal_accumulate(img, f, cam, history=dict(history, length=np.zeros((4, 6))))
    with pytest.raises(ValueError, match="of one 5x4 frame"):
        render.temporal_accumulate(img, dict(f, depth=np.zeros((3, 5))), cam)
    for kw, name in (({"max_history": 65536}, "max_history"), ({"max_history": -1}, "max_history"), ({"depth_tolerance": -1.0}, "depth_tolerance"),
                     ({"depth_tolerance": float("nan")}, "depth_tolerance"), ({"normal_min": 1.5}, "normal_min"),
                     ({"normal_min": float("nan")}, "normal_min")):
        with pytest.raises(ValueError, match=name):
            render.temporal_accumulate(img, f, cam, **kw)
    with pytest.raises(ValueError, match="at least one frame"):
        render.orbit_cameras(cam, 0, 1.0)


def test_the_orbit_ends_at_the_given_camera():
    """Frame k's lookfrom is the camera's, turned about the axis through lookat along view_up by (k - (K - 1)) * step degrees."""
    from rttnw_amd import scene as S
    cam = S.camera_desc(lookfrom=(3.0, 2.0, 4.0), lookat=(1.0, 0.5, 0.0), vfov=40.0, aspect=1.0, view_up=(0.0, 2.0, 0.0))
    cams = render.orbit_cameras(cam, 4, 90.0)
    assert bytes(cams[3]) == bytes(cam)
    arm = np.array([2.0, 1.5, 4.0])
    for k, want in ((2, (-4.0, 1.5, 2.0)), (1, (-2.0, 1.5, -4.0)), (0, (4.0, 1.5, -2.0))):       # -90, -180, -270 degrees about +y
        got = np.array(cams[k].lookfrom[:]) - np.array(cam.lookat[:])
        assert np.abs(got - np.array(want)).max() < 1e-12, (k, got)
        assert abs(np.sqrt(got @ got) - np.sqrt(arm @ arm)) < 1e-12
        assert cams[k].lookat[:] == cam.lookat[:] and cams[k].vertical_fov == cam.vertical_fov and cams[k].focus_distance == cam.focus_distance


@pytest.mark.parametrize("argv,msg", [
    (["7", "--temporal"], "--temporal needs --orbit"),
    (["7", "--orbit", "3", "--noise", "0.1"], "--orbit does not combine with --noise"),
    (["7", "--orbit", "3", "--window", "0,0,8,8"], "--orbit does not combine with --window"),
    (["7", "--orbit", "3", "--devices", "0,0"], "--orbit does not combine with --devices"),
    (["7", "--orbit", "3", "--denoise-nlm"], "--orbit does not combine with --denoise-nlm"),
    (["7", "--orbit", "3", "--temporal", "--denoise-select"], "--orbit does not combine with --denoise-select"),
    (["7", "--orbit", "0", "--temporal"], "--orbit must be 1 .. 1000"),
    (["7", "--orbit", "3", "--orbit-step", "nan"], "--orbit-step must be -360 .. 360"),
    (["7", "--orbit", "3", "--denoise", "--denoise-iterations", "9"], "--denoise-iterations must be 0 .. 8"),
])
def test_cli_refuses_before_any_scene_is_built(argv, msg, tmp_path):
    cli_refuses(argv, msg, tmp_path, must_not_exist=("frame_000.png",))
