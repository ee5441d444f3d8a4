"""rttnw_render_adaptive_multi without a GPU: the export exists and is declared alike in the header, the ctypes binding and the Rust binding,
every argument refusal comes before the device is touched and in the order the header states, and the command line refuses a malformed
--devices and its combinations before any scene is built.  (The fourth refusal, a device id outside [0, rttnw_device_count()), stands behind
validate() and so behind "scene is not committed": tests/test_gpu_adaptive_multi.py has it, on a committed scene.)"""
import ctypes as C

import pytest

from abi_cases import HEADER_TEXT, INVALID, RUST_SCENE, STATE, UNSUPPORTED, camera, cli_refuses, declared_alike, exported, refused
from abi_cases import adaptive as _adaptive, params as _params
from rttnw_amd import abi, library
from rttnw_amd import scene as S

NAME = "render_adaptive_multi"

# the argument list, once: (name, C type, Rust type, ctypes type)
ARGS = [("s", "rttnw_scene*", "*mut rttnw_scene", abi.scene_p),
        ("cam", "const rttnw_camera_desc*", "*const rttnw_camera_desc", C.POINTER(abi.CameraDesc)),
        ("p", "const rttnw_params*", "*const rttnw_params", C.POINTER(abi.Params)),
        ("a", "const rttnw_adaptive*", "*const rttnw_adaptive", C.POINTER(abi.Adaptive)),
        ("ngpu", "uint32_t", "u32", C.c_uint32),
        ("device_ids", "const int32_t*", "*const i32", C.POINTER(C.c_int32)),
        ("out_linear_rgb", "double*", "*mut f64", C.c_void_p), ("out_rgba8", "uint8_t*", "*mut u8", C.c_void_p),
        ("out_spp", "uint32_t*", "*mut u32", C.c_void_p), ("out_stderr_rgb", "double*", "*mut f64", C.c_void_p),
        ("stats", "rttnw_stats*", "*mut rttnw_stats", C.c_void_p)]


def test_export_and_declarations():
    exported(NAME)
    declared_alike(NAME, ARGS)
    assert "rttnw_" + NAME in HEADER_TEXT.split("typedef struct rttnw_scene")[0], "the comment at RTTNW_ABI_VERSION says how a caller detects the function"
    assert NAME in RUST_SCENE, "the crate's safe wrapper"


def _call(b, sc, p, a, ngpu=2, ids=(0, 0), scene=True):
    cam = camera()
    dev = None if ids is None else (C.c_int32 * max(len(ids), 1))(*ids)
    return b.render_adaptive_multi(sc.handle if scene else None, C.byref(cam), C.byref(p) if p is not None else None,
                                   C.byref(a) if a is not None else None, ngpu, dev, None, None, None, None, None)


@pytest.mark.parametrize("what,kw,adapt,call,code,msg", [
    # 1. the multi form's own arguments
    ("NULL p", None, {}, {}, INVALID, "NULL"),
    ("NULL a", {}, None, {}, INVALID, "NULL"),
    ("ngpu 0", {}, {}, {"ngpu": 0}, INVALID, "ngpu"),
    ("ngpu 65", {}, {}, {"ngpu": 65, "ids": (0,) * 65}, INVALID, "ngpu"),
    ("NULL device_ids", {}, {}, {"ids": None}, INVALID, "device_ids"),
    # 2. what rttnw_render_adaptive refuses among its own arguments, with its codes
    ("pass_spp 0", {}, {"pass_spp": 0}, {}, INVALID, "pass_spp is 0"),
    ("cap not a multiple", {"spp": 96}, {}, {}, INVALID, "multiple of pass_spp"),
    ("cap 0", {"spp": 0}, {}, {}, INVALID, "multiple of pass_spp"),
    ("negative rel", {}, {"rel_error": -0.1}, {}, INVALID, "rel_error and abs_error"),
    ("NaN abs", {}, {"abs_error": float("nan")}, {}, INVALID, "rel_error and abs_error"),
    ("reserved0", {}, {"reserved0": 1}, {}, INVALID, "reserved0"),
    ("counters", {"collect_counters": 1}, {}, {}, UNSUPPORTED, "collect_counters"),
    # 3. validate()
    ("empty image", {"width": 0}, {}, {}, None, "empty image"),
    ("bad precision", {"precision": 9}, {}, {}, None, "precision"),
    ("negative t_min", {"t_min": -1.0}, {}, {}, None, "t_min"),
])
def test_refusals_come_before_the_device(what, kw, adapt, call, code, msg):
    b = library.product()
    sc = S.Scene(b)                                   # never committed: a device would be needed for that
    p = None if kw is None else _params(**kw)
    a = None if adapt is None else _adaptive(**adapt)
    refused(b, lambda scene: _call(b, sc, p, a, scene=scene, **call), code, msg, NAME)


def test_tile_rank_and_tile_world_are_ignored():
    """The single call's tile_world rule is the one refusal the multi form does not share: the caller's partition fields are not read."""
    b = library.product()
    sc = S.Scene(b)
    assert _call(b, sc, _params(tile_world=2, tile_rank=1), _adaptive()) == STATE and "not committed" in b.last_error().decode()
    assert _call(b, sc, _params(tile_world=0, tile_rank=7), _adaptive()) == STATE


def test_refusals_come_in_the_stated_order():
    """A call that breaks two rules returns the earlier one's code and message."""
    b = library.product()
    sc = S.Scene(b)
    err = lambda: b.last_error().decode()
    # 1 before 2
    assert _call(b, sc, _params(), _adaptive(pass_spp=0), ngpu=0) == INVALID and "ngpu" in err()
    assert _call(b, sc, _params(collect_counters=1), _adaptive(), ids=None) == INVALID and "device_ids" in err()
    assert _call(b, sc, None, _adaptive(reserved0=1), ngpu=0) == INVALID and "NULL" in err()
    # inside 2: the single call's order — pass_spp, the cap, the tolerances, reserved0, collect_counters
    assert _call(b, sc, _params(spp=96), _adaptive(pass_spp=0)) == INVALID and "pass_spp is 0" in err()
    assert _call(b, sc, _params(spp=96), _adaptive(rel_error=-1.0)) == INVALID and "multiple of pass_spp" in err()
    assert _call(b, sc, _params(), _adaptive(rel_error=-1.0, reserved0=1)) == INVALID and "rel_error" in err()
    assert _call(b, sc, _params(collect_counters=1), _adaptive(reserved0=1)) == INVALID and "reserved0" in err()
    # 2 before 3: collect_counters before what rttnw_render refuses — an empty image, a bad precision, a NULL or uncommitted scene
    assert _call(b, sc, _params(collect_counters=1, width=0), _adaptive()) == UNSUPPORTED and "collect_counters" in err()
    assert _call(b, sc, _params(collect_counters=1, precision=9), _adaptive(), scene=False) == UNSUPPORTED
    # 3 before 4: a device id nobody has is not looked at while the scene is not committed
    assert _call(b, sc, _params(), _adaptive(), ids=(0, 1 << 20)) == STATE and "not committed" in err()
    assert _call(b, sc, _params(), _adaptive(), ids=(-1, 0), scene=False) == INVALID and "NULL" in err()
    # ... and valid arguments reach those checks
    assert _call(b, sc, _params(), _adaptive()) == STATE and "not committed" in err()
    assert _call(b, sc, _params(), _adaptive(), ngpu=64, ids=(0,) * 64) == STATE
    assert _call(b, sc, _params(), _adaptive(), scene=False) == INVALID and "NULL" in err()


@pytest.mark.parametrize("argv,msg", [
    (["7", "--devices", ""], "--devices wants D0,D1,..."),
    (["7", "--devices", "0,,1"], "--devices wants D0,D1,..."),
    (["7", "--devices", "0,x"], "--devices wants D0,D1,..."),
    (["7", "--devices", "0,-1"], "--devices wants D0,D1,..."),
    (["7", "--devices", ",".join(["0"] * 65)], "--devices wants D0,D1,..."),
    (["7", "--devices", "0,0", "--window", "0,0,8,8"], "--devices does not combine with --window"),
    (["7", "--devices", "0,0", "--features", "f"], "--devices does not combine with --features"),
    (["7", "--devices", "0,0", "--denoise"], "--devices does not combine with --denoise"),
    (["7", "--devices", "0,0", "--passes", "2"], "--devices does not combine with --passes"),
    (["7", "--devices", "0,0", "--noise", "0.05", "--denoise"], "--devices does not combine with --denoise"),
])
def test_cli_refuses_before_any_scene_is_built(argv, msg, tmp_path):
    cli_refuses(argv, msg, tmp_path)
