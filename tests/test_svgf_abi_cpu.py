"""rttnw_svgf_create / _destroy / _reset / _push / _frame without a GPU: the exports exist and are declared alike in the header, the ctypes
binding and the Rust binding; rttnw_svgf_params and rttnw_svgf_out have one layout in all three; the header states the contract; every
argument refusal comes before the device is touched, with a message that names the call and the argument; a valid create without a device
fails loudly; the Python driver and the command line refuse what they must before the library is called.  (tests/test_svgf_cpu.py has the
arithmetic, tests/test_gpu_svgf.py what the device computes — and the one refusal that needs a handle, a frame of another size.)"""
import ctypes as C
import re

import numpy as np
import pytest

from abi_cases import FFI, HEADER, HEADER_TEXT, INVALID, camera, cli_refuses, declared_alike, exported
from rttnw_amd import abi, library, render
from rttnw_amd import scene as S

_CD = ("const double*", "*const f64", C.c_void_p)
_CAM = ("const rttnw_camera_desc*", "*const rttnw_camera_desc", C.POINTER(abi.CameraDesc))
_Q = ("rttnw_svgf*", "*mut rttnw_svgf", C.c_void_p)
_OUT = ("const rttnw_svgf_out*", "*const rttnw_svgf_out", C.POINTER(abi.SvgfOut))
HIP = -4


def test_exports_and_declarations():
    for name in ("svgf_create", "svgf_destroy", "svgf_reset", "svgf_push", "svgf_frame"):
        exported(name)
    declared_alike("svgf_create", [("width", "uint32_t", "u32", C.c_uint32), ("height", "uint32_t", "u32", C.c_uint32),
                                   ("q", "const rttnw_svgf_params*", "*const rttnw_svgf_params", C.POINTER(abi.Svgf)),
                                   ("out", "rttnw_svgf**", "*mut *mut rttnw_svgf", C.POINTER(C.c_void_p))])
    declared_alike("svgf_reset", [("q",) + _Q])
    declared_alike("svgf_push", [("q",) + _Q, ("cam",) + _CAM] + [(n,) + _CD for n in ("linear_rgb", "albedo", "normal", "depth", "alpha")] + [("out",) + _OUT])
    declared_alike("svgf_frame", [("q",) + _Q, ("s", "rttnw_scene*", "*mut rttnw_scene", abi.scene_p), ("cam",) + _CAM,
                                  ("p", "const rttnw_params*", "*const rttnw_params", C.POINTER(abi.Params)), ("out",) + _OUT,
                                  ("stats", "rttnw_stats*", "*mut rttnw_stats", C.POINTER(abi.Stats))])
    assert re.search(r"\bvoid rttnw_svgf_destroy\(rttnw_svgf\* q\);", HEADER) and re.search(r"pub fn rttnw_svgf_destroy\(q: \*mut rttnw_svgf\);", FFI)
    assert re.search(r"typedef struct rttnw_svgf rttnw_svgf;", HEADER)
    assert "rttnw_svgf_create" in HEADER_TEXT.split("typedef struct rttnw_scene")[0], "the comment at RTTNW_ABI_VERSION says how a caller detects the feature"


def _rust_fields(name):
    attrs, body = re.search(r"((?:#\[[^\]]*\]\s*)+)pub struct %s\s*\{(.*?)\n\}" % name, FFI, flags=re.S).groups()
    assert "repr(C)" in attrs
    return re.findall(r"pub (\w+)\s*:\s*([^,\n]+),", body)


def test_struct_layouts_agree_in_header_ctypes_and_rust():
    body = re.search(r"struct rttnw_svgf_params \{(.*?)\};", HEADER, flags=re.S).group(1)
    assert [" ".join(d.split()) for d in body.split(";") if d.strip()] == [
        "uint32_t feedback_iterations", "uint32_t demodulate", "uint32_t feature_spp", "uint32_t reserved0", "rttnw_temporal_params t",
        "rttnw_variance_params v", "rttnw_denoise_params d"]
    assert re.search(r"typedef struct rttnw_svgf_params rttnw_svgf_params;", HEADER) and re.search(r"typedef struct rttnw_svgf_out rttnw_svgf_out;", HEADER)
    fields = [("feedback_iterations", "u32", C.c_uint32), ("demodulate", "u32", C.c_uint32), ("feature_spp", "u32", C.c_uint32),
              ("reserved0", "u32", C.c_uint32), ("t", "rttnw_temporal_params", abi.Temporal), ("v", "rttnw_variance_params", abi.Variance),
              ("d", "rttnw_denoise_params", abi.Denoise)]
    assert _rust_fields("rttnw_svgf_params") == [(n, r) for n, r, _ in fields]
    assert list(abi.Svgf._fields_) == [(n, t) for n, _, t in fields]
    assert C.sizeof(abi.Svgf) == 104 and [getattr(abi.Svgf, n).offset for n, _, _ in fields] == [0, 4, 8, 12, 16, 40, 72]
    body = re.search(r"struct rttnw_svgf_out \{(.*?)\};", HEADER, flags=re.S).group(1)
    c_fields = [" ".join(d.split()) for d in body.split(";") if d.strip()]
    assert c_fields == [("uint8_t* " if n == "rgba8" else "double* ") + n for n in abi.SVGF_OUTPUTS]
    assert _rust_fields("rttnw_svgf_out") == [(n, "*mut u8" if n == "rgba8" else "*mut f64") for n in abi.SVGF_OUTPUTS]
    assert [n for n, _ in abi.SvgfOut._fields_] == list(abi.SVGF_OUTPUTS) and C.sizeof(abi.SvgfOut) == 8 * 16
    assert set(render.SVGF_ARRAYS) | {"image_ms"} == set(abi.SVGF_OUTPUTS)


def test_the_header_states_the_contract():
    contract = HEADER_TEXT.split("typedef struct rttnw_svgf rttnw_svgf;")[0].split("int rttnw_temporal_variance(", 1)[1]
    contract = re.sub(r"\n \*\s*", " ", contract)
    for phrase in ("The contract is a composition of the existing entry points", "empty after rttnw_svgf_create and after rttnw_svgf_reset",
                   "c = C / albedo", "rttnw_denoise's rule", "A1 is an albedo map of all 1.0", "prev_linear_rgb = M1, prev_moment2_rgb = M2, prev_length = L",
                   "the no-history call", "prev_linear_rgb = H", "the taps are the same", "Otherwise A = M1",
                   "rttnw_denoise(A, var, A1, F.normal, F.depth, F.alpha, d)", "with iterations = j", "a tap of the pass loop, not a second run",
                   "With j = 0 no H is kept", "linear_rgb = D * albedo on the channels step 0 divided", "main.rs:219-225 with alpha 255",
                   "in the filter's units", "rttnw_svgf_frame is rttnw_svgf_push of rttnw_render's out_linear_rgb", "min(p->spp, 16)",
                   "no product is fused into a sum", "non-finite values are not special-cased", "give the same bits",
                   "var is the variance of the raw running mean M1, not of the cleaner A", "conservative", "No CPU fallback",
                   "allocate nothing in a frame call", "waits once", "an output that is NULL is not copied", "feedback_iterations > d.iterations",
                   "demodulate > 1", "reserved0 != 0", "a size that differs from the handle's or tile_world != 1", "Out of scope", "a node-wide form",
                   "adaptive sampling inside the sequence", "colour clamping of the history", "the non-local-means and select filters", "the native rttnw program",
                   "moving geometry"):
        assert phrase in contract, phrase


def _params(**kw):
    q = abi.Svgf(feedback_iterations=0, demodulate=0, feature_spp=0, reserved0=0, t=abi.Temporal(), v=abi.Variance(), d=abi.Denoise(iterations=3))
    for key, val in kw.items():
        block, _, field = key.partition("__")
        if field:
            setattr(getattr(q, block), field, val)
        else:
            setattr(q, key, val)
    return q


def _create(b, drop=(), width=4, height=3, **kw):
    q, out = _params(**kw), C.c_void_p()
    rc = b.svgf_create(width, height, None if "q" in drop else C.byref(q), None if "out" in drop else C.byref(out))
    assert not out.value or rc == 0
    if out.value:
        b.svgf_destroy(out)
    return rc


NAN = float("nan")
CREATE_REFUSALS = [
    ("NULL q", {"drop": ("q",)}, "q is NULL"),
    ("NULL out", {"drop": ("out",)}, "out is NULL"),
    ("width 0", {"width": 0}, "width * height"),
    ("height 0", {"height": 0}, "width * height"),
    ("max_history 65536", {"t__max_history": 65536}, "t.max_history"),
    ("t's reserved0", {"t__reserved0": 1}, "t.reserved0"),
    ("negative depth_tolerance", {"t__depth_tolerance": -0.1}, "t.depth_tolerance"),
    ("NaN depth_tolerance", {"t__depth_tolerance": NAN}, "t.depth_tolerance"),
    ("normal_min 1.5", {"t__normal_min": 1.5}, "t.normal_min"),
    ("NaN normal_min", {"t__normal_min": NAN}, "t.normal_min"),
    ("min_temporal 1", {"v__min_temporal": 1}, "v.min_temporal"),
    ("min_temporal 65536", {"v__min_temporal": 65536}, "v.min_temporal"),
    ("radius 5", {"v__radius": 5}, "v.radius"),
    ("v's reserved0", {"v__reserved0": 1}, "v.reserved0"),
    ("v's reserved1", {"v__reserved1": 7}, "v.reserved1"),
    ("negative v.sigma_normal", {"v__sigma_normal": -1.0}, "v.sigma_normal"),
    ("NaN v.sigma_depth", {"v__sigma_depth": NAN}, "v.sigma_depth"),
    ("9 iterations", {"d__iterations": 9}, "d.iterations"),
    ("d's reserved0", {"d__reserved0": 1}, "d.reserved0"),
    ("negative sigma_luminance", {"d__sigma_luminance": -1.0}, "d.sigma_luminance"),
    ("NaN d.sigma_normal", {"d__sigma_normal": NAN}, "sigma_normal"),
    ("negative d.sigma_depth", {"d__sigma_depth": -2.0}, "sigma_depth"),
    ("feedback above iterations", {"feedback_iterations": 4}, "feedback_iterations"),
    ("feedback without passes", {"feedback_iterations": 1, "d__iterations": 0}, "feedback_iterations"),
    ("demodulate 2", {"demodulate": 2}, "demodulate"),
    ("reserved0", {"reserved0": 1}, "q->reserved0"),
]


@pytest.mark.parametrize("what,kw,msg", CREATE_REFUSALS, ids=[r[0] for r in CREATE_REFUSALS])
def test_create_refuses_before_the_device(what, kw, msg):
    b = library.product()
    assert _create(b, **kw) == INVALID, what
    err = b.last_error().decode()
    assert err.startswith("svgf_create:") and msg in err, (what, err)


def _push(b, drop=()):
    arr = {k: np.ones(36) for k in ("linear_rgb", "albedo", "normal", "depth", "alpha")}
    cam = camera()
    return b.svgf_push(None, None if "cam" in drop else C.byref(cam), *[None if k in drop else arr[k].ctypes.data for k in arr], None)


@pytest.mark.parametrize("drop,msg", [(("cam",), "cam is NULL"), (("linear_rgb",), "linear_rgb"), (("albedo",), "albedo"), (("normal",), "normal"),
                                      (("depth",), "depth"), (("alpha",), "alpha"), ((), "q is NULL")])
def test_push_refuses_before_the_device(drop, msg):
    """(out itself may be NULL: it is in every call here)"""
    b = library.product()
    assert _push(b, drop) == INVALID
    err = b.last_error().decode()
    assert err.startswith("svgf_push:") and msg in err, err


def test_frame_and_reset_refuse_before_the_device():
    b = library.product()
    cam, p = camera(), S.make_params(16, 16, 4)
    for args, msg in (((None, None, None, C.byref(p), None, None), "cam is NULL"), ((None, None, C.byref(cam), None, None, None), "p is NULL"),
                      ((None, None, C.byref(cam), C.byref(p), None, None), "q is NULL")):
        assert b.svgf_frame(*args) == INVALID
        assert b.last_error().decode().startswith("svgf_frame:") and msg in b.last_error().decode(), b.last_error().decode()
    p.tile_world, p.tile_rank = 2, 0
    assert b.svgf_frame(None, None, C.byref(cam), C.byref(p), None, None) == INVALID
    assert b.last_error().decode().startswith("svgf_frame:") and "tile_world" in b.last_error().decode()
    assert b.svgf_reset(None) == INVALID and b.last_error().decode().startswith("svgf_reset:") and "q is NULL" in b.last_error().decode()
    b.svgf_destroy(None)                                                  # a NULL handle is destroyed like free(NULL)


@pytest.mark.skipif(library.product().device_count() > 0, reason="a GPU is present")
@pytest.mark.parametrize("kw", [{}, {"feedback_iterations": 3, "demodulate": 1}, {"v__radius": 4, "v__min_temporal": 2}, {"d__iterations": 0}])
def test_a_valid_create_without_a_device_fails_loudly(kw):
    b = library.product()
    assert _create(b, **kw) == HIP
    assert "no CPU fallback" in b.last_error().decode() and "svgf_create" in b.last_error().decode()


def test_the_python_driver_refuses_before_the_library_is_called():
    for kw, name in (({"feedback": 6}, "feedback"), ({"feedback": -1}, "feedback"), ({"iterations": 9}, "iterations")):
        with pytest.raises(ValueError, match=name):
            render.SvgfSequence(8, 8, **kw)
    with pytest.raises(ValueError, match="width and height"):
        render.SvgfSequence(0, 8)


@pytest.mark.parametrize("argv,msg", [
    (["7", "--svgf"], "--svgf needs --orbit"),
    (["7", "--orbit", "3", "--feedback", "1"], "--feedback and --demodulate need --svgf"),
    (["7", "--orbit", "3", "--demodulate"], "--feedback and --demodulate need --svgf"),
    (["7", "--orbit", "3", "--svgf", "--feedback", "6"], "--feedback must be 0 .. --denoise-iterations"),
    (["7", "--orbit", "3", "--svgf", "--noise", "0.1"], "--orbit does not combine with --noise"),
    (["7", "--orbit", "3", "--svgf", "--denoise-select"], "--orbit does not combine with --denoise-select"),
    (["7", "--orbit", "3", "--svgf", "--devices", "0,0"], "--orbit does not combine with --devices"),
    (["7", "--orbit", "0", "--svgf"], "--orbit must be 1 .. 1000"),
])
def test_cli_refuses_before_any_scene_is_built(argv, msg, tmp_path):
    cli_refuses(argv, msg, tmp_path, must_not_exist=("frame_000.png",))
