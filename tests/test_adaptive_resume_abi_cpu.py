"""rttnw_render_adaptive_resume without a GPU: both exports exist and are declared alike in the header, the ctypes binding and the Rust binding;
rttnw_adaptive_state_doubles counts what the header says; every argument refusal — the state's checks included — comes before the device is
touched and in the order the header states; and the command line refuses --resume / --save-state where they mean nothing, before any scene is
built.  (The sixth refusal, a device id outside [0, rttnw_device_count()), stands behind validate() and so behind "scene is not committed":
tests/test_gpu_adaptive_resume.py has the refusals of a committed scene.)"""
import ctypes as C
import re

import numpy as np
import pytest

from abi_cases import (CAM, HEADER, HEADER_TEXT, INVALID, MAGIC, RUST_SCENE, STATE, STATE_HEADER_DOUBLES, STATE_RECORD_DOUBLES, UNSUPPORTED, VERSION,
                       chunks_of_a_pass, cli_refuses, declared_alike, exported, refused)
from abi_cases import adaptive as _adaptive, break_state as _break, hand_made_state as _state, params as _params
from rttnw_amd import abi, library
from rttnw_amd import scene as S

# the argument list, once: (name, C type, Rust type, ctypes type)
ARGS = [("s", "rttnw_scene*", "*mut rttnw_scene", abi.scene_p),
        ("cam", "const rttnw_camera_desc*", "*const rttnw_camera_desc", C.POINTER(abi.CameraDesc)),
        ("p", "const rttnw_params*", "*const rttnw_params", C.POINTER(abi.Params)),
        ("a", "const rttnw_adaptive*", "*const rttnw_adaptive", C.POINTER(abi.Adaptive)),
        ("ngpu", "uint32_t", "u32", C.c_uint32),
        ("device_ids", "const int32_t*", "*const i32", C.POINTER(C.c_int32)),
        ("state_in", "const double*", "*const f64", C.c_void_p), ("state_out", "double*", "*mut f64", C.c_void_p),
        ("out_linear_rgb", "double*", "*mut f64", C.c_void_p), ("out_rgba8", "uint8_t*", "*mut u8", C.c_void_p),
        ("out_spp", "uint32_t*", "*mut u32", C.c_void_p), ("out_stderr_rgb", "double*", "*mut f64", C.c_void_p),
        ("stats", "rttnw_stats*", "*mut rttnw_stats", C.c_void_p)]
SIZE_ARGS = [("width", "uint32_t", "u32", C.c_uint32), ("height", "uint32_t", "u32", C.c_uint32)]


def test_exports_and_declarations():
    for name in ("render_adaptive_resume", "adaptive_state_doubles"):
        exported(name)
    declared_alike("render_adaptive_resume", ARGS)
    declared_alike("adaptive_state_doubles", SIZE_ARGS, "uint64_t", "u64", C.c_uint64)
    assert "rttnw_render_adaptive_resume" in HEADER_TEXT.split("typedef struct rttnw_scene")[0], \
        "the comment at RTTNW_ABI_VERSION says how a caller detects the function"
    assert "render_adaptive_resume" in RUST_SCENE, "the crate's safe wrapper"
    assert "does NOT identify the scene" in HEADER_TEXT, "the header says what the state does not check"
    for name, val in (("MAGIC", MAGIC), ("VERSION", VERSION), ("HEADER", STATE_HEADER_DOUBLES), ("RECORD", STATE_RECORD_DOUBLES)):
        assert re.search(r"#define RTTNW_ADAPTIVE_STATE_%s %du\b" % (name, val), HEADER), name


@pytest.mark.parametrize("w,h", [(1, 1), (40, 24), (45, 37), (0, 7), (7, 0), (0, 0), (65535, 65535)])
def test_state_doubles(w, h):
    assert library.product().adaptive_state_doubles(w, h) == 64 + 12 * w * h


def _call(b, sc, p, a, ngpu=2, ids=(0, 0), scene=True, state=None, cam=None):
    cam = S.camera_desc(**CAM) if cam is None else cam
    dev = None if ids is None else (C.c_int32 * max(len(ids), 1))(*ids)
    return b.render_adaptive_resume(sc.handle if scene else None, C.byref(cam), C.byref(p) if p is not None else None,
                                    C.byref(a) if a is not None else None, ngpu, dev, None if state is None else state.ctypes.data,
                                    None, None, None, None, None, None)


@pytest.mark.parametrize("what,kw,adapt,call,code,msg", [
    # 1. NULL p or a
    ("NULL p", None, {}, {}, INVALID, "NULL"),
    ("NULL a", {}, None, {}, INVALID, "NULL"),
    # 2. where it runs
    ("ngpu 65", {}, {}, {"ngpu": 65, "ids": (0,) * 65}, INVALID, "ngpu"),
    ("NULL device_ids", {}, {}, {"ids": None}, INVALID, "device_ids"),
    ("device_ids with ngpu 0", {}, {}, {"ngpu": 0, "ids": (0,)}, INVALID, "device_ids"),
    # 3. what rttnw_render_adaptive refuses among its own arguments, with its codes
    ("pass_spp 0", {}, {"pass_spp": 0}, {}, INVALID, "pass_spp is 0"),
    ("cap not a multiple", {"spp": 96}, {}, {}, INVALID, "multiple of pass_spp"),
    ("cap 0", {"spp": 0}, {}, {}, INVALID, "multiple of pass_spp"),
    ("negative rel", {}, {"rel_error": -0.1}, {}, INVALID, "rel_error and abs_error"),
    ("NaN abs", {}, {"abs_error": float("nan")}, {}, INVALID, "rel_error and abs_error"),
    ("reserved0", {}, {"reserved0": 1}, {}, INVALID, "reserved0"),
    ("counters", {"collect_counters": 1}, {}, {}, UNSUPPORTED, "collect_counters"),
    ("tile_world with ngpu 0", {"tile_world": 2}, {}, {"ngpu": 0, "ids": None}, INVALID, "tile_world"),
    # 5. validate()
    ("empty image", {"width": 0}, {}, {}, None, "empty image"),
    ("bad precision", {"precision": 9}, {}, {}, None, "precision"),
    ("negative t_min", {"t_min": -1.0}, {}, {}, None, "t_min"),
])
def test_refusals_come_before_the_device(what, kw, adapt, call, code, msg):
    b = library.product()
    sc = S.Scene(b)                                   # never committed: a device would be needed for that
    p = None if kw is None else _params(**kw)
    a = None if adapt is None else _adaptive(**adapt)
    refused(b, lambda scene: _call(b, sc, p, a, scene=scene, **call), code, msg, "render_adaptive_resume")


def test_tile_fields_are_ignored_with_ranks_and_the_single_form_reaches_validate():
    b = library.product()
    sc = S.Scene(b)
    assert _call(b, sc, _params(tile_world=2, tile_rank=1), _adaptive()) == STATE and "not committed" in b.last_error().decode()
    assert _call(b, sc, _params(), _adaptive(), ngpu=0, ids=None) == STATE and "not committed" in b.last_error().decode()
    assert _call(b, sc, _params(), _adaptive(), ngpu=64, ids=(0,) * 64) == STATE


# 4. the state: (what is broken, header index or (record field, value), the word the message must hold)
STATE_BREAKS = [("magic", 0, "magic"), ("version", 1, "version"), ("width", 2, "width"), ("height", 3, "height"), ("pass_spp", 4, "pass_spp"),
                ("spp_chunk", 5, "spp_chunk"), ("sample_begin", 6, "sample_begin"), ("precision", 7, "precision"), ("max_depth", 8, "max_depth"),
                ("quirks", 9, "quirks"), ("seed low", 10, "seed"), ("seed high", 11, "seed"), ("t_min", 12, "t_min"),
                ("background r", 13, "background"), ("background b", 15, "background"), ("lookfrom x", 16, "lookfrom"), ("lookat z", 21, "lookat"),
                ("view_up y", 23, "view_up"), ("vertical_fov", 25, "vertical_fov"), ("aspect_ratio", 26, "aspect_ratio"), ("aperture", 27, "aperture"),
                ("focus_distance", 28, "focus_distance"), ("open_time", 29, "open_time"), ("close_time", 30, "close_time"),
                ("n NaN", ("n", float("nan")), "n is not a finite integer"), ("n inf", ("n", float("inf")), "n is not a finite integer"),
                ("n 0", ("n", 0.0), "below pass_spp"), ("n B + 1", ("n", 65.0), "multiple of pass_spp"),
                ("n cap + B", ("n", 192.0), "the state holds more samples than the cap"), ("k wrong", ("k", 15.0), "k is not"),
                ("k NaN", ("k", float("nan")), "k is not a finite integer"), ("k for two passes", ("k", 32.0), "k is not")]


def test_a_valid_state_reaches_validate():
    b = library.product()
    sc = S.Scene(b)
    p, a, cam = _params(spp_chunk=4), _adaptive(), S.camera_desc(**CAM)
    st = _state(p, a, cam)
    for call in ({}, {"ngpu": 0, "ids": None}):
        assert _call(b, sc, p, a, state=st, **call) == STATE and "not committed" in b.last_error().decode()
        assert _call(b, sc, p, a, state=st, scene=False, **call) == INVALID and "NULL" in b.last_error().decode()
    # records at two passes and at the cap are as valid
    assert _call(b, sc, p, a, state=_state(p, a, cam, n=128, k=32)) == STATE


@pytest.mark.parametrize("name,what,msg", STATE_BREAKS, ids=[x[0] for x in STATE_BREAKS])
def test_a_broken_state_is_refused_before_the_scene_is_looked_at(name, what, msg):
    b = library.product()
    sc = S.Scene(b)
    p, a, cam = _params(spp_chunk=4), _adaptive(), S.camera_desc(**CAM)
    st = _break(_state(p, a, cam), what)
    for scene in (True, False):
        assert _call(b, sc, p, a, state=st, scene=scene) == INVALID, name
        err = b.last_error().decode()
        assert msg in err and "render_adaptive_resume" in err and "not committed" not in err, (name, err)


def test_header_fields_are_compared_bitwise():
    """-0.0 against 0.0 in the background differs; a NaN t_min equals itself (and is then refused by validate(), behind the scene's state)."""
    b = library.product()
    sc = S.Scene(b)
    p, a, cam = _params(), _adaptive(), S.camera_desc(**CAM)
    st = _state(p, a, cam)
    st[14] = -0.0
    assert _call(b, sc, p, a, state=st) == INVALID and "background" in b.last_error().decode()
    p = _params(t_min=float("nan"))
    assert _call(b, sc, p, a, state=_state(p, a, cam)) == STATE and "not committed" in b.last_error().decode()


def test_records_are_not_looked_at_without_pixels():
    b = library.product()
    sc = S.Scene(b)
    a, cam = _adaptive(), S.camera_desc(**CAM)
    for kw in ({"width": 0}, {"height": 0}):
        p = _params(**kw)
        st = np.full(64 + 12, np.nan)                 # whatever stands behind the header
        st[:64] = _state(p, a, cam)[:64]
        assert _call(b, sc, p, a, state=st) == STATE and "not committed" in b.last_error().decode()
        st[2 if "width" in kw else 3] = 5.0           # ... but the header is
        assert _call(b, sc, p, a, state=st) == INVALID and ("width" if "width" in kw else "height") in b.last_error().decode()


@pytest.mark.parametrize("B,spp_chunk,expected", [(32, 0, 11), (64, 4, 16), (16, 2, 8), (16, 0, 16), (33, 4, 9)])
def test_chunk_counts_of_the_validation(B, spp_chunk, expected):
    b = library.product()
    sc = S.Scene(b)
    assert chunks_of_a_pass(B, spp_chunk) == expected
    p, a, cam = _params(spp=4 * B, spp_chunk=spp_chunk), _adaptive(pass_spp=B), S.camera_desc(**CAM)
    assert _call(b, sc, p, a, state=_state(p, a, cam)) == STATE and "not committed" in b.last_error().decode()
    assert _call(b, sc, p, a, state=_state(p, a, cam, n=3 * B, k=3 * expected)) == STATE
    assert _call(b, sc, p, a, state=_state(p, a, cam, k=expected + 1)) == INVALID and "k is not" in b.last_error().decode()


def test_refusals_come_in_the_stated_order():
    """A call that breaks two rules returns the earlier one's code and message."""
    b = library.product()
    sc = S.Scene(b)
    err = lambda: b.last_error().decode()
    p, a, cam = _params(), _adaptive(), S.camera_desc(**CAM)
    good = _state(p, a, cam)
    bad = _break(good, 0)
    # 1 before 2
    assert _call(b, sc, None, _adaptive(), ngpu=65, ids=(0,) * 65) == INVALID and "NULL" in err()
    assert _call(b, sc, _params(), None, ngpu=0, ids=(0,)) == INVALID and "NULL" in err()
    # 2 before 3
    assert _call(b, sc, _params(), _adaptive(pass_spp=0), ngpu=65, ids=(0,) * 65) == INVALID and "ngpu" in err()
    assert _call(b, sc, _params(collect_counters=1), _adaptive(), ids=None) == INVALID and "device_ids" in err()
    assert _call(b, sc, _params(spp=96), _adaptive(), ngpu=0, ids=(0,)) == INVALID and "device_ids" in err()
    # inside 3: the single call's order — pass_spp, the cap, the tolerances, reserved0, tile_world (ngpu == 0), collect_counters
    assert _call(b, sc, _params(spp=96), _adaptive(pass_spp=0)) == INVALID and "pass_spp is 0" in err()
    assert _call(b, sc, _params(spp=96), _adaptive(rel_error=-1.0)) == INVALID and "multiple of pass_spp" in err()
    assert _call(b, sc, _params(), _adaptive(rel_error=-1.0, reserved0=1)) == INVALID and "rel_error" in err()
    assert _call(b, sc, _params(collect_counters=1), _adaptive(reserved0=1)) == INVALID and "reserved0" in err()
    assert _call(b, sc, _params(collect_counters=1, tile_world=2), _adaptive(), ngpu=0, ids=None) == INVALID and "tile_world" in err()
    # 3 before 4: a bad state is not looked at while the adaptive arguments are wrong
    assert _call(b, sc, _params(collect_counters=1), _adaptive(), state=bad) == UNSUPPORTED and "collect_counters" in err()
    assert _call(b, sc, _params(), _adaptive(reserved0=1), state=bad) == INVALID and "reserved0" in err()
    assert _call(b, sc, _params(tile_world=2), _adaptive(), ngpu=0, ids=None, state=bad) == INVALID and "tile_world" in err()
    # inside 4: magic, version, the header in its order, then the records
    assert _call(b, sc, p, a, state=_break(bad, 1)) == INVALID and "magic" in err()
    assert _call(b, sc, p, a, state=_break(_break(good, 1), 2)) == INVALID and "version" in err()
    assert _call(b, sc, p, a, state=_break(_break(good, 10), 4)) == INVALID and "pass_spp" in err()
    assert _call(b, sc, p, a, state=_break(_break(good, 30), ("n", 0.0))) == INVALID and "close_time" in err()
    st = _break(good, ("n", 192.0))
    st[64 + 5 * 12 + 7] = float("nan")
    assert _call(b, sc, p, a, state=st) == INVALID and "k is not a finite integer" in err()
    # 4 before 5: the state before an empty image, a bad precision, a NULL or uncommitted scene
    pe = _params(height=0)
    assert _call(b, sc, pe, a, state=_break(_state(pe, a, cam), 0)) == INVALID and "magic" in err()
    pp = _params(precision=9)
    assert _call(b, sc, pp, a, state=_break(_state(pp, a, cam), ("n", 65.0)), scene=False) == INVALID and "multiple of pass_spp" in err()
    assert _call(b, sc, p, a, state=bad, scene=False) == INVALID and "magic" in err()
    # 5 before 6: a device id nobody has is not looked at while the scene is not committed
    assert _call(b, sc, p, a, ids=(0, 1 << 20), state=good) == STATE and "not committed" in err()
    assert _call(b, sc, p, a, ids=(-1, 0), scene=False) == INVALID and "NULL" in err()


@pytest.mark.parametrize("argv,msg", [
    (["7", "--resume", "state.npy"], "--resume needs --noise"),
    (["7", "--save-state", "state.npy"], "--save-state needs --noise"),
    (["7", "--devices", "0,0", "--resume", "state.npy"], "--resume needs --noise"),
    (["7", "--noise", "0.1", "--resume", "state.npy", "--passes", "2"], "--resume does not combine with --passes"),
    (["7", "--noise", "0.1", "--save-state", "state.npy", "--passes", "2"], "--save-state does not combine with --passes"),
    (["7", "--resume", "state.npy", "--window", "0,0,8,8"], "--resume needs --noise"),
    (["7", "--noise", "0.1", "--resume", "state.npy", "--window", "0,0,8,8"], "--resume does not combine with --window"),
    (["7", "--noise", "0.1", "--save-state", "state.npy", "--window", "0,0,8,8"], "--save-state does not combine with --window"),
])
def test_cli_refuses_before_any_scene_is_built(argv, msg, tmp_path):
    cli_refuses(argv, msg, tmp_path, must_not_exist=("state.npy",))
