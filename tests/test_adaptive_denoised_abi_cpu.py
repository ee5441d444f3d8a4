"""rttnw_render_adaptive_denoised without a GPU: the export exists and is declared alike in the header, the ctypes binding and the Rust binding;
rttnw_guided is 8 bytes followed by rttnw_denoise_params in all three; every argument refusal comes before the device is touched — on a scene
that was never committed, and on no scene at all — in the order the header states, with a message that names the entry point and the field; and
the command line refuses --guided where it means nothing, before any scene is built.  (tests/test_gpu_adaptive_denoised.py has what a
committed scene computes.)"""
import ctypes as C
import re

import pytest

from abi_cases import FFI, HEADER, HEADER_TEXT, INVALID, RUST_SCENE, STATE, UNSUPPORTED, camera, cli_refuses, declared_alike, exported, refused
from abi_cases import adaptive as _adaptive, params as _params
from rttnw_amd import abi, library
from rttnw_amd import scene as S

NAME = "render_adaptive_denoised"

# the argument list, once: (name, C type, Rust type, ctypes type)
ARGS = [("s", "rttnw_scene*", "*mut rttnw_scene", abi.scene_p),
        ("cam", "const rttnw_camera_desc*", "*const rttnw_camera_desc", C.POINTER(abi.CameraDesc)),
        ("p", "const rttnw_params*", "*const rttnw_params", C.POINTER(abi.Params)),
        ("a", "const rttnw_adaptive*", "*const rttnw_adaptive", C.POINTER(abi.Adaptive)),
        ("g", "const rttnw_guided*", "*const rttnw_guided", C.POINTER(abi.Guided)),
        ("out_linear_rgb", "double*", "*mut f64", C.c_void_p), ("out_rgba8", "uint8_t*", "*mut u8", C.c_void_p),
        ("out_spp", "uint32_t*", "*mut u32", C.c_void_p), ("out_stderr_rgb", "double*", "*mut f64", C.c_void_p),
        ("out_raw_linear_rgb", "double*", "*mut f64", C.c_void_p), ("out_raw_stderr_rgb", "double*", "*mut f64", C.c_void_p),
        ("state_out", "double*", "*mut f64", C.c_void_p),
        ("stats", "rttnw_stats*", "*mut rttnw_stats", C.POINTER(abi.Stats))]


def test_export_and_declarations():
    exported(NAME)
    declared_alike(NAME, ARGS)
    assert "rttnw_" + NAME in HEADER_TEXT.split("typedef struct rttnw_scene")[0], "the comment at RTTNW_ABI_VERSION says how a caller detects the function"
    assert "pub fn %s(" % NAME in RUST_SCENE, "the crate's safe wrapper"
    contract = HEADER_TEXT.split("struct rttnw_guided {")[0].split("int rttnw_render_adaptive_region(", 1)[1]
    assert "NOT promised" in contract, "the header says that a stopped pixel's decision depended on its neighbours"
    assert "Out of scope: a node-wide form" in contract and "state_in" in contract and "windows" in contract


def test_guided_layout_agrees_in_header_ctypes_and_rust():
    """rttnw_guided = two 32-bit words, then rttnw_denoise_params: 8 + sizeof(rttnw_denoise_params) bytes, the same fields in the same order."""
    body = re.search(r"struct rttnw_guided \{(.*?)\};", HEADER, flags=re.S).group(1)
    c_fields = [tuple(" ".join(d.split()).rsplit(" ", 1)) for d in body.split(";") if d.strip()]
    assert c_fields == [("uint32_t", "feature_spp"), ("uint32_t", "reserved0"), ("rttnw_denoise_params", "denoise")]
    assert re.search(r"typedef struct rttnw_guided rttnw_guided;", HEADER)
    attrs, rs_body = re.search(r"((?:#\[[^\]]*\]\s*)+)pub struct rttnw_guided\s*\{(.*?)\n\}", FFI, flags=re.S).groups()
    assert "repr(C)" in attrs
    assert re.findall(r"pub (\w+)\s*:\s*(\w+),", rs_body) == [("feature_spp", "u32"), ("reserved0", "u32"), ("denoise", "rttnw_denoise_params")]
    assert [(n, t) for n, t in abi.Guided._fields_] == [("feature_spp", C.c_uint32), ("reserved0", C.c_uint32), ("denoise", abi.Denoise)]
    assert C.sizeof(abi.Denoise) == 32 and C.sizeof(abi.Guided) == 8 + C.sizeof(abi.Denoise)
    assert abi.Guided.feature_spp.offset == 0 and abi.Guided.reserved0.offset == 4 and abi.Guided.denoise.offset == 8
    # ... and rttnw_denoise_params itself is the struct rttnw_denoise takes, in the header and in Rust
    d_body = re.search(r"struct rttnw_denoise_params \{(.*?)\};", HEADER, flags=re.S).group(1)
    assert [n.strip() for d in d_body.split(";") if d.strip() for n in d.split(None, 1)[1].split(",")] == [f[0] for f in abi.Denoise._fields_]
    rs_d = re.search(r"pub struct rttnw_denoise_params\s*\{(.*?)\n\}", FFI, flags=re.S).group(1)
    assert [n for n, _ in re.findall(r"pub (\w+)\s*:\s*(\w+),", rs_d)] == [f[0] for f in abi.Denoise._fields_]


def _guided(**kw):
    g = abi.Guided(feature_spp=0, reserved0=0, denoise=abi.Denoise(iterations=5, reserved0=0, sigma_luminance=0.0, sigma_normal=0.0, sigma_depth=0.0))
    for k, v in kw.items():
        if k.startswith("denoise_"):
            setattr(g.denoise, k[len("denoise_"):], v)
        else:
            setattr(g, k, v)
    return g


def _call(b, sc, p, a, g, scene=True):
    cam = camera()
    return b.render_adaptive_denoised(sc.handle if scene else None, C.byref(cam), C.byref(p) if p is not None else None,
                                      C.byref(a) if a is not None else None, C.byref(g) if g is not None else None, None, None, None, None, None, None,
                                      None, None)


@pytest.mark.parametrize("what,kw,adapt,guide,code,msg", [
    # 1. NULL p, a or g
    ("NULL p", None, {}, {}, INVALID, "NULL"),
    ("NULL a", {}, None, {}, INVALID, "NULL"),
    ("NULL g", {}, {}, None, INVALID, "NULL"),
    # 2. what rttnw_render_adaptive refuses among its own arguments, with its codes
    ("pass_spp 0", {}, {"pass_spp": 0}, {}, INVALID, "pass_spp is 0"),
    ("cap not a multiple", {"spp": 96}, {}, {}, INVALID, "multiple of pass_spp"),
    ("cap 0", {"spp": 0}, {}, {}, INVALID, "multiple of pass_spp"),
    ("negative rel", {}, {"rel_error": -0.1}, {}, INVALID, "rel_error and abs_error"),
    ("NaN abs", {}, {"abs_error": float("nan")}, {}, INVALID, "rel_error and abs_error"),
    ("a->reserved0", {}, {"reserved0": 1}, {}, INVALID, "reserved0"),
    ("tile_world", {"tile_world": 2}, {}, {}, INVALID, "tile_world"),
    ("counters", {"collect_counters": 1}, {}, {}, UNSUPPORTED, "collect_counters"),
    # 3. the guide's own fields
    ("g->reserved0", {}, {}, {"reserved0": 1}, INVALID, "g->reserved0"),
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
def test_refusals_come_before_the_device(what, kw, adapt, guide, code, msg):
    b = library.product()
    sc = S.Scene(b)                                   # never committed: a device would be needed for that
    p = None if kw is None else _params(**kw)
    a = None if adapt is None else _adaptive(**adapt)
    g = None if guide is None else _guided(**guide)
    refused(b, lambda scene: _call(b, sc, p, a, g, scene=scene), code, msg, NAME)


def test_valid_arguments_reach_validate():
    """Every value the contract allows — 0 and 8 iterations, a feature_spp of its own, sigmas of the caller's — passes the call's own checks."""
    b = library.product()
    sc = S.Scene(b)
    for guide in ({}, {"denoise_iterations": 0}, {"denoise_iterations": 8}, {"feature_spp": 7},
                  {"denoise_sigma_luminance": 2.0, "denoise_sigma_normal": 128.0, "denoise_sigma_depth": 0.5}):
        assert _call(b, sc, _params(), _adaptive(), _guided(**guide)) == STATE and "not committed" in b.last_error().decode(), guide
    assert _call(b, sc, _params(spp=64), _adaptive(rel_error=0.0), _guided()) == STATE      # cap == B, a tolerance of 0


def test_refusals_come_in_the_stated_order():
    """A call that breaks two rules returns the earlier one's code and message."""
    b = library.product()
    sc = S.Scene(b)
    err = lambda: b.last_error().decode()
    # 1 before 2 and 3
    assert _call(b, sc, None, _adaptive(pass_spp=0), _guided(reserved0=1)) == INVALID and "NULL" in err()
    assert _call(b, sc, _params(spp=96), None, _guided()) == INVALID and "NULL" in err()
    assert _call(b, sc, _params(spp=96), _adaptive(), None) == INVALID and "NULL" in err()
    # inside 2: the single call's order — pass_spp, the cap, the tolerances, reserved0, tile_world, collect_counters
    assert _call(b, sc, _params(spp=96), _adaptive(pass_spp=0), _guided()) == INVALID and "pass_spp is 0" in err()
    assert _call(b, sc, _params(spp=96), _adaptive(rel_error=-1.0), _guided()) == INVALID and "multiple of pass_spp" in err()
    assert _call(b, sc, _params(), _adaptive(rel_error=-1.0, reserved0=1), _guided()) == INVALID and "rel_error" in err()
    assert _call(b, sc, _params(tile_world=2), _adaptive(reserved0=1), _guided()) == INVALID and "reserved0" in err() and "g->" not in err()
    assert _call(b, sc, _params(collect_counters=1, tile_world=2), _adaptive(), _guided()) == INVALID and "tile_world" in err()
    # 2 before 3
    assert _call(b, sc, _params(collect_counters=1), _adaptive(), _guided(reserved0=1)) == UNSUPPORTED and "collect_counters" in err()
    assert _call(b, sc, _params(), _adaptive(abs_error=-1.0), _guided(denoise_iterations=9)) == INVALID and "rel_error and abs_error" in err()
    # inside 3: g->reserved0, iterations, denoise.reserved0, the sigmas
    assert _call(b, sc, _params(), _adaptive(), _guided(reserved0=1, denoise_iterations=9)) == INVALID and "g->reserved0" in err()
    assert _call(b, sc, _params(), _adaptive(), _guided(denoise_iterations=9, denoise_reserved0=1)) == INVALID and "denoise.iterations" in err()
    assert _call(b, sc, _params(), _adaptive(), _guided(denoise_reserved0=1, denoise_sigma_depth=-1.0)) == INVALID and "denoise.reserved0" in err()
    # 3 before 4: the guide before a bad precision, a NULL or uncommitted scene
    assert _call(b, sc, _params(precision=9), _adaptive(), _guided(denoise_sigma_depth=-1.0)) == INVALID and "sigma_depth" in err()
    assert _call(b, sc, _params(), _adaptive(), _guided(reserved0=1), scene=False) == INVALID and "g->reserved0" in err()
    assert _call(b, sc, _params(precision=9), _adaptive(), _guided()) == STATE and "not committed" in err()


@pytest.mark.parametrize("argv,msg", [
    (["7", "--guided"], "--guided needs --noise"),
    (["7", "--guided", "--denoise"], "--guided needs --noise"),
    (["7", "--noise", "0.1", "--guided", "--devices", "0,0"], "--guided does not combine with --devices"),
    (["7", "--noise", "0.1", "--guided", "--resume", "state.npy"], "--guided does not combine with --resume"),
    (["7", "--noise", "0.1", "--guided", "--refine", "0,0,8,8"], "--guided does not combine with --refine"),
    (["7", "--noise", "0.1", "--guided", "--passes", "2"], "--guided does not combine with --passes"),
    (["7", "--noise", "0.1", "--guided", "--denoise-iterations", "9"], "--denoise-iterations must be 0 .. 8"),
])
def test_cli_refuses_before_any_scene_is_built(argv, msg, tmp_path):
    cli_refuses(argv, msg, tmp_path, must_not_exist=("state.npy",))
