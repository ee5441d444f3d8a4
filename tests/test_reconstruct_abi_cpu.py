"""rttnw_reconstruct and rttnw_render_preview without a GPU: the exports exist and are declared alike in the header, the ctypes binding and the
Rust binding; rttnw_preview is 8 bytes followed by rttnw_denoise_params in all three; every argument refusal comes before the device is touched —
on a scene that was never committed, and on no scene at all — in the order the header states, with a message that names the entry point and the
field; and the command line refuses --preview where it means nothing, before any scene is built.  (tests/test_gpu_reconstruct.py and
tests/test_gpu_preview.py have what the device computes.)"""
import ctypes as C
import re

import numpy as np
import pytest

from abi_cases import FFI, HEADER, HEADER_TEXT, INVALID, RUST_SCENE, STATE, UNSUPPORTED, camera, cli_refuses, declared_alike, exported, refused
from abi_cases import adaptive as _adaptive, params as _params
from rttnw_amd import abi, library, render
from rttnw_amd import scene as S

# the argument lists, once: (name, C type, Rust type, ctypes type)
_D, _U8, _U32 = ("double*", "*mut f64", C.c_void_p), ("uint8_t*", "*mut u8", C.c_void_p), ("uint32_t*", "*mut u32", C.c_void_p)
_CD, _CU8 = ("const double*", "*const f64", C.c_void_p), ("const uint8_t*", "*const u8", C.c_void_p)
ARGS = {
    "reconstruct": [("width", "uint32_t", "u32", C.c_uint32), ("height", "uint32_t", "u32", C.c_uint32), ("linear_rgb",) + _CD, ("variance_rgb",) + _CD,
                    ("valid",) + _CU8, ("albedo",) + _CD, ("normal",) + _CD, ("depth",) + _CD, ("alpha",) + _CD,
                    ("d", "const rttnw_denoise_params*", "*const rttnw_denoise_params", C.POINTER(abi.Denoise)),
                    ("out_linear_rgb",) + _D, ("out_rgba8",) + _U8, ("out_variance_rgb",) + _D, ("out_valid",) + _U8,
                    ("kernel_ms", "double*", "*mut f64", C.POINTER(C.c_double))],
    "render_preview": [("s", "rttnw_scene*", "*mut rttnw_scene", abi.scene_p),
                       ("cam", "const rttnw_camera_desc*", "*const rttnw_camera_desc", C.POINTER(abi.CameraDesc)),
                       ("p", "const rttnw_params*", "*const rttnw_params", C.POINTER(abi.Params)),
                       ("a", "const rttnw_adaptive*", "*const rttnw_adaptive", C.POINTER(abi.Adaptive)),
                       ("v", "const rttnw_preview*", "*const rttnw_preview", C.POINTER(abi.Preview)),
                       ("out_linear_rgb",) + _D, ("out_rgba8",) + _U8, ("out_valid",) + _U8, ("out_spp",) + _U32, ("out_raw_linear_rgb",) + _D,
                       ("out_raw_stderr_rgb",) + _D, ("state_out",) + _D, ("stats", "rttnw_stats*", "*mut rttnw_stats", C.POINTER(abi.Stats))],
}


@pytest.mark.parametrize("name", ["reconstruct", "render_preview"])
def test_export_and_declarations(name):
    exported(name)
    declared_alike(name, ARGS[name])
    assert "rttnw_" + name in HEADER_TEXT.split("typedef struct rttnw_scene")[0], "the comment at RTTNW_ABI_VERSION says how a caller detects the function"
    assert "pub fn %s(" % name in RUST_SCENE, "the crate's safe wrapper"


def test_the_header_says_what_the_preview_leaves_out_and_why_its_features_take_the_pass_size():
    contract = HEADER_TEXT.split("struct rttnw_preview {")[0].split("int rttnw_reconstruct(", 1)[1]
    assert "Out of scope: a state_in" in contract and "ngpu" in contract and "windows" in contract
    assert "feature_spp defaults to the pass size" in contract and "albedo" in contract
    assert "NO variance goes into the filter" in contract
    text = HEADER_TEXT.split("int rttnw_reconstruct(", 1)[0].split("int rttnw_render_adaptive_denoised(", 1)[1]
    assert "NEVER READ" in text and "bit for bit" in text


def test_preview_layout_agrees_in_header_ctypes_and_rust():
    """rttnw_preview = two 32-bit words, then rttnw_denoise_params: 8 + sizeof(rttnw_denoise_params) bytes, the same fields in the same order."""
    body = re.search(r"struct rttnw_preview \{(.*?)\};", HEADER, flags=re.S).group(1)
    c_fields = [tuple(" ".join(d.split()).rsplit(" ", 1)) for d in body.split(";") if d.strip()]
    assert c_fields == [("uint32_t", "level"), ("uint32_t", "feature_spp"), ("rttnw_denoise_params", "denoise")]
    assert re.search(r"typedef struct rttnw_preview rttnw_preview;", HEADER)
    attrs, rs_body = re.search(r"((?:#\[[^\]]*\]\s*)+)pub struct rttnw_preview\s*\{(.*?)\n\}", FFI, flags=re.S).groups()
    assert "repr(C)" in attrs
    assert re.findall(r"pub (\w+)\s*:\s*(\w+),", rs_body) == [("level", "u32"), ("feature_spp", "u32"), ("denoise", "rttnw_denoise_params")]
    assert [(n, t) for n, t in abi.Preview._fields_] == [("level", C.c_uint32), ("feature_spp", C.c_uint32), ("denoise", abi.Denoise)]
    assert C.sizeof(abi.Denoise) == 32 and C.sizeof(abi.Preview) == 8 + C.sizeof(abi.Denoise)
    assert abi.Preview.level.offset == 0 and abi.Preview.feature_spp.offset == 4 and abi.Preview.denoise.offset == 8


def test_lattice_mask():
    m = render.lattice_mask(45, 37, 2)
    assert m.shape == (37, 45) and m.dtype == np.uint8 and m.sum() == 12 * 10
    ys, xs = np.nonzero(m)
    assert (ys % 4 == 0).all() and (xs % 4 == 0).all() and m[0, 0] == 1 and m[36, 44] == 1
    assert render.lattice_mask(5, 3, 0).all() and render.lattice_mask(45, 37, 6).sum() == 1
    with pytest.raises(ValueError):
        render.lattice_mask(8, 8, 7)


# ---------------------------------------------------------------- rttnw_reconstruct's refusals

def _reconstruct_call(b, drop=(), width=4, height=3, **dkw):
    n = width * height
    arr = {"linear_rgb": np.zeros(max(n, 1) * 3), "variance_rgb": np.zeros(max(n, 1) * 3), "valid": np.ones(max(n, 1), dtype=np.uint8),
           "albedo": np.zeros(max(n, 1) * 3), "normal": np.zeros(max(n, 1) * 3), "depth": np.zeros(max(n, 1)), "alpha": np.zeros(max(n, 1))}
    d = abi.Denoise(iterations=5, reserved0=0, sigma_luminance=0.0, sigma_normal=0.0, sigma_depth=0.0)
    for k, v in dkw.items():
        setattr(d, k, v)
    ptr = lambda k: None if k in drop else arr[k].ctypes.data
    return b.reconstruct(width, height, ptr("linear_rgb"), ptr("variance_rgb"), ptr("valid"), ptr("albedo"), ptr("normal"), ptr("depth"), ptr("alpha"),
                         None if "d" in drop else C.byref(d), None, None, None, None, None)


@pytest.mark.parametrize("what,kw,msg", [
    ("NULL linear_rgb", {"drop": ("linear_rgb",)}, "linear_rgb"),
    ("NULL albedo", {"drop": ("albedo",)}, "albedo"),
    ("NULL normal", {"drop": ("normal",)}, "normal"),
    ("NULL depth", {"drop": ("depth",)}, "depth"),
    ("NULL alpha", {"drop": ("alpha",)}, "alpha"),
    ("NULL d", {"drop": ("d",)}, "NULL"),
    ("NULL valid", {"drop": ("valid",)}, "valid is NULL"),
    ("empty image", {"width": 0}, "width * height"),
    ("iterations 9", {"iterations": 9}, "iterations"),
    ("reserved0", {"reserved0": 1}, "reserved0"),
    ("negative sigma_luminance", {"sigma_luminance": -1.0}, "sigma_luminance"),
    ("NaN sigma_normal", {"sigma_normal": float("nan")}, "sigma_normal"),
    ("negative sigma_depth", {"sigma_depth": -0.5}, "sigma_depth"),
])
def test_reconstruct_refusals_come_before_the_device(what, kw, msg):
    b = library.product()
    assert _reconstruct_call(b, **kw) == INVALID, what
    err = b.last_error().decode()
    assert err.startswith("reconstruct:") and msg in err, (what, err)


def test_reconstruct_refusals_come_in_rttnw_denoise_order():
    b = library.product()
    err = lambda: b.last_error().decode()
    assert _reconstruct_call(b, drop=("albedo", "valid"), width=0) == INVALID and "albedo" in err()       # rttnw_denoise's NULLs first
    assert _reconstruct_call(b, drop=("valid",), width=0, iterations=9) == INVALID and "valid is NULL" in err()
    assert _reconstruct_call(b, width=0, iterations=9) == INVALID and "width * height" in err()
    assert _reconstruct_call(b, iterations=9, reserved0=1) == INVALID and "iterations" in err()
    assert _reconstruct_call(b, reserved0=1, sigma_depth=-1.0) == INVALID and "reserved0" in err()


# ---------------------------------------------------------------- rttnw_render_preview's refusals

NAME = "render_preview"
def _preview(**kw):
    v = abi.Preview(level=2, feature_spp=0, denoise=abi.Denoise(iterations=5, reserved0=0, sigma_luminance=0.0, sigma_normal=0.0, sigma_depth=0.0))
    for k, val in kw.items():
        if k.startswith("denoise_"):
            setattr(v.denoise, k[len("denoise_"):], val)
        else:
            setattr(v, k, val)
    return v


def _call(b, sc, p, a, v, scene=True):
    cam = camera()
    return b.render_preview(sc.handle if scene else None, C.byref(cam), C.byref(p) if p is not None else None, C.byref(a) if a is not None else None,
                            C.byref(v) if v is not None else None, None, None, None, None, None, None, None, None)


@pytest.mark.parametrize("what,kw,adapt,prev,code,msg", [
    # 1. NULL p, a or v
    ("NULL p", None, {}, {}, INVALID, "NULL"),
    ("NULL a", {}, None, {}, INVALID, "NULL"),
    ("NULL v", {}, {}, None, INVALID, "NULL"),
    # 2. what rttnw_render_adaptive refuses among its own arguments, with its codes
    ("pass_spp 0", {}, {"pass_spp": 0}, {}, INVALID, "pass_spp is 0"),
    ("cap not a multiple", {"spp": 96}, {}, {}, INVALID, "multiple of pass_spp"),
    ("cap 0", {"spp": 0}, {}, {}, INVALID, "multiple of pass_spp"),
    ("negative rel", {}, {"rel_error": -0.1}, {}, INVALID, "rel_error and abs_error"),
    ("NaN abs", {}, {"abs_error": float("nan")}, {}, INVALID, "rel_error and abs_error"),
    ("a->reserved0", {}, {"reserved0": 1}, {}, INVALID, "reserved0"),
    ("tile_world", {"tile_world": 2}, {}, {}, INVALID, "tile_world"),
    ("counters", {"collect_counters": 1}, {}, {}, UNSUPPORTED, "collect_counters"),
    # 3. the preview's own fields
    ("level 7", {}, {}, {"level": 7}, INVALID, "v->level"),
    ("iterations 9", {}, {}, {"denoise_iterations": 9}, INVALID, "denoise.iterations"),
    ("denoise.reserved0", {}, {}, {"denoise_reserved0": 1}, INVALID, "denoise.reserved0"),
    ("negative sigma_luminance", {}, {}, {"denoise_sigma_luminance": -1.0}, INVALID, "sigma_luminance"),
    ("NaN sigma_normal", {}, {}, {"denoise_sigma_normal": float("nan")}, INVALID, "sigma_normal"),
    ("negative sigma_depth", {}, {}, {"denoise_sigma_depth": -0.5}, INVALID, "sigma_depth"),
    # 4. validate()
    ("bad precision", {"precision": 9}, {}, {}, None, "precision"),
    ("negative t_min", {"t_min": -1.0}, {}, {}, None, "t_min"),
    ("empty image", {"width": 0}, {}, {}, None, "empty image"),
])
def test_preview_refusals_come_before_the_device(what, kw, adapt, prev, code, msg):
    b = library.product()
    sc = S.Scene(b)                                   # never committed: a device would be needed for that
    p = None if kw is None else _params(**kw)
    a = None if adapt is None else _adaptive(**adapt)
    v = None if prev is None else _preview(**prev)
    refused(b, lambda scene: _call(b, sc, p, a, v, scene=scene), code, msg, NAME)


def test_valid_preview_arguments_reach_validate():
    """Every value the contract allows — levels 0 and 6, 0 and 8 iterations, a feature_spp of its own, sigmas of the caller's — passes the call's own checks."""
    b = library.product()
    sc = S.Scene(b)
    for prev in ({}, {"level": 0}, {"level": 6}, {"denoise_iterations": 0}, {"denoise_iterations": 8}, {"feature_spp": 7},
                 {"denoise_sigma_luminance": 2.0, "denoise_sigma_normal": 128.0, "denoise_sigma_depth": 0.5}):
        assert _call(b, sc, _params(), _adaptive(), _preview(**prev)) == STATE and "not committed" in b.last_error().decode(), prev
    assert _call(b, sc, _params(spp=64), _adaptive(rel_error=0.0), _preview()) == STATE      # cap == B, a tolerance of 0


def test_preview_refusals_come_in_the_stated_order():
    """A call that breaks two rules returns the earlier one's code and message."""
    b = library.product()
    sc = S.Scene(b)
    err = lambda: b.last_error().decode()
    # 1 before 2 and 3
    assert _call(b, sc, None, _adaptive(pass_spp=0), _preview(level=7)) == INVALID and "NULL" in err()
    assert _call(b, sc, _params(spp=96), None, _preview()) == INVALID and "NULL" in err()
    assert _call(b, sc, _params(spp=96), _adaptive(), None) == INVALID and "NULL" in err()
    # inside 2: the single call's order — pass_spp, the cap, the tolerances, reserved0, tile_world, collect_counters
    assert _call(b, sc, _params(spp=96), _adaptive(pass_spp=0), _preview()) == INVALID and "pass_spp is 0" in err()
    assert _call(b, sc, _params(spp=96), _adaptive(rel_error=-1.0), _preview()) == INVALID and "multiple of pass_spp" in err()
    assert _call(b, sc, _params(), _adaptive(rel_error=-1.0, reserved0=1), _preview()) == INVALID and "rel_error" in err()
    assert _call(b, sc, _params(tile_world=2), _adaptive(reserved0=1), _preview()) == INVALID and "reserved0" in err() and "v->" not in err()
    assert _call(b, sc, _params(collect_counters=1, tile_world=2), _adaptive(), _preview()) == INVALID and "tile_world" in err()
    # 2 before 3
    assert _call(b, sc, _params(collect_counters=1), _adaptive(), _preview(level=7)) == UNSUPPORTED and "collect_counters" in err()
    assert _call(b, sc, _params(), _adaptive(abs_error=-1.0), _preview(denoise_iterations=9)) == INVALID and "rel_error and abs_error" in err()
    # inside 3: the level, iterations, denoise.reserved0, the sigmas
    assert _call(b, sc, _params(), _adaptive(), _preview(level=7, denoise_iterations=9)) == INVALID and "v->level" in err()
    assert _call(b, sc, _params(), _adaptive(), _preview(denoise_iterations=9, denoise_reserved0=1)) == INVALID and "denoise.iterations" in err()
    assert _call(b, sc, _params(), _adaptive(), _preview(denoise_reserved0=1, denoise_sigma_depth=-1.0)) == INVALID and "denoise.reserved0" in err()
    # 3 before 4: the preview's fields before a bad precision, a NULL or uncommitted scene
    assert _call(b, sc, _params(precision=9), _adaptive(), _preview(denoise_sigma_depth=-1.0)) == INVALID and "sigma_depth" in err()
    assert _call(b, sc, _params(), _adaptive(), _preview(level=7), scene=False) == INVALID and "v->level" in err()
    assert _call(b, sc, _params(precision=9), _adaptive(), _preview()) == STATE and "not committed" in err()


@pytest.mark.parametrize("argv,msg", [
    (["7", "--preview", "2"], "--preview needs --noise"),
    (["7", "--preview", "2", "--denoise"], "--preview needs --noise"),
    (["7", "--noise", "0.1", "--preview", "2", "--devices", "0,0"], "--preview does not combine with --devices"),
    (["7", "--noise", "0.1", "--preview", "2", "--resume", "state.npy"], "--preview does not combine with --resume"),
    (["7", "--noise", "0.1", "--preview", "2", "--refine", "0,0,8,8"], "--preview does not combine with --refine"),
    (["7", "--noise", "0.1", "--preview", "2", "--guided"], "--preview does not combine with --guided"),
    (["7", "--noise", "0.1", "--preview", "2", "--passes", "2"], "--preview does not combine with --passes"),
    (["7", "--noise", "0.1", "--preview", "7"], "--preview must be 0 .. 6"),
    (["7", "--noise", "0.1", "--preview", "2", "--denoise-iterations", "9"], "--denoise-iterations must be 0 .. 8"),
])
def test_cli_refuses_before_any_scene_is_built(argv, msg, tmp_path):
    cli_refuses(argv + ["--save-state", str(tmp_path / "saved.npy")], msg, tmp_path, must_not_exist=("saved.npy",))
