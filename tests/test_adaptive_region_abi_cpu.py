"""rttnw_render_adaptive_region without a GPU: the export exists and is declared alike in the header, the ctypes binding and the Rust binding; every
argument refusal — the window's, the state's checks with their one addition (a record of twelve zeros is a pixel without samples) — comes before
the device is touched and in the order the header states; rttnw_render_adaptive_resume still refuses such a state with the message it always
had; and the command line refuses --refine where it means nothing, before any scene is built.  (The seventh refusal, a device id outside
[0, rttnw_device_count()), stands behind validate() and so behind "scene is not committed": tests/test_gpu_adaptive_region.py has the refusals
of a committed scene.)"""
import ctypes as C

import pytest

from abi_cases import HEADER_TEXT, INVALID, RUST_SCENE, STATE, UNSUPPORTED, camera, cli_refuses, declared_alike, exported, refused
from abi_cases import adaptive as _adaptive, break_state as _break, hand_made_state as _state, params as _params
from rttnw_amd import abi, library
from rttnw_amd import scene as S

NAME = "render_adaptive_region"

# the argument list, once: (name, C type, Rust type, ctypes type)
ARGS = [("s", "rttnw_scene*", "*mut rttnw_scene", abi.scene_p),
        ("cam", "const rttnw_camera_desc*", "*const rttnw_camera_desc", C.POINTER(abi.CameraDesc)),
        ("p", "const rttnw_params*", "*const rttnw_params", C.POINTER(abi.Params)),
        ("a", "const rttnw_adaptive*", "*const rttnw_adaptive", C.POINTER(abi.Adaptive)),
        ("x0", "uint32_t", "u32", C.c_uint32), ("y0", "uint32_t", "u32", C.c_uint32),
        ("x1", "uint32_t", "u32", C.c_uint32), ("y1", "uint32_t", "u32", C.c_uint32),
        ("mask", "const uint8_t*", "*const u8", C.c_void_p),
        ("ngpu", "uint32_t", "u32", C.c_uint32),
        ("device_ids", "const int32_t*", "*const i32", C.POINTER(C.c_int32)),
        ("state_in", "const double*", "*const f64", C.c_void_p), ("state_out", "double*", "*mut f64", C.c_void_p),
        ("out_linear_rgb", "double*", "*mut f64", C.c_void_p), ("out_rgba8", "uint8_t*", "*mut u8", C.c_void_p),
        ("out_spp", "uint32_t*", "*mut u32", C.c_void_p), ("out_stderr_rgb", "double*", "*mut f64", C.c_void_p),
        ("stats", "rttnw_stats*", "*mut rttnw_stats", C.c_void_p)]


def test_export_and_declarations():
    exported(NAME)
    declared_alike(NAME, ARGS)
    assert "rttnw_" + NAME in HEADER_TEXT.split("typedef struct rttnw_scene")[0], "the comment at RTTNW_ABI_VERSION says how a caller detects the function"
    assert "pub fn %s(" % NAME in RUST_SCENE, "the crate's safe wrapper"
    assert "A window-sized state is out of scope" in HEADER_TEXT, "the header says what scales with the frame"


W, H = 16, 16
WIN = (3, 5, 12, 11)


def _call(b, sc, p, a, win=WIN, ngpu=2, ids=(0, 0), scene=True, state=None, cam=None, resume=False):
    cam = camera() if cam is None else cam
    dev = None if ids is None else (C.c_int32 * max(len(ids), 1))(*ids)
    head = (sc.handle if scene else None, C.byref(cam), C.byref(p) if p is not None else None, C.byref(a) if a is not None else None)
    tail = (ngpu, dev, None if state is None else state.ctypes.data, None, None, None, None, None, None)
    if resume:
        return b.render_adaptive_resume(*head, *tail)
    return b.render_adaptive_region(*head, *win, None, *tail)


@pytest.mark.parametrize("what,kw,adapt,call,code,msg", [
    # 1. NULL p or a
    ("NULL p", None, {}, {}, INVALID, "NULL"),
    ("NULL a", {}, None, {}, INVALID, "NULL"),
    # 2. the window
    ("x0 == x1", {}, {}, {"win": (5, 5, 5, 11)}, INVALID, "window"),
    ("y0 > y1", {}, {}, {"win": (3, 12, 12, 11)}, INVALID, "window"),
    ("x1 > width", {}, {}, {"win": (3, 5, W + 1, 11)}, INVALID, "window"),
    ("y1 > height", {}, {}, {"win": (3, 5, 12, H + 1)}, INVALID, "window"),
    # 3. where it runs
    ("ngpu 65", {}, {}, {"ngpu": 65, "ids": (0,) * 65}, INVALID, "ngpu"),
    ("NULL device_ids", {}, {}, {"ids": None}, INVALID, "device_ids"),
    ("device_ids with ngpu 0", {}, {}, {"ngpu": 0, "ids": (0,)}, INVALID, "device_ids"),
    # 4. what rttnw_render_adaptive refuses among its own arguments, with its codes
    ("pass_spp 0", {}, {"pass_spp": 0}, {}, INVALID, "pass_spp is 0"),
    ("cap not a multiple", {"spp": 96}, {}, {}, INVALID, "multiple of pass_spp"),
    ("cap 0", {"spp": 0}, {}, {}, INVALID, "multiple of pass_spp"),
    ("negative rel", {}, {"rel_error": -0.1}, {}, INVALID, "rel_error and abs_error"),
    ("NaN abs", {}, {"abs_error": float("nan")}, {}, INVALID, "rel_error and abs_error"),
    ("reserved0", {}, {"reserved0": 1}, {}, INVALID, "reserved0"),
    ("counters", {"collect_counters": 1}, {}, {}, UNSUPPORTED, "collect_counters"),
    ("tile_world with ngpu 0", {"tile_world": 2}, {}, {"ngpu": 0, "ids": None}, INVALID, "tile_world"),
    # 6. validate()
    ("bad precision", {"precision": 9}, {}, {}, None, "precision"),
    ("negative t_min", {"t_min": -1.0}, {}, {}, None, "t_min"),
])
def test_refusals_come_before_the_device(what, kw, adapt, call, code, msg):
    b = library.product()
    sc = S.Scene(b)                                   # never committed: a device would be needed for that
    p = None if kw is None else _params(**kw)
    a = None if adapt is None else _adaptive(**adapt)
    refused(b, lambda scene: _call(b, sc, p, a, scene=scene, **call), code, msg, NAME)


def test_tile_fields_are_ignored_with_ranks_and_the_single_form_reaches_validate():
    b = library.product()
    sc = S.Scene(b)
    assert _call(b, sc, _params(tile_world=2, tile_rank=1), _adaptive()) == STATE and "not committed" in b.last_error().decode()
    assert _call(b, sc, _params(), _adaptive(), ngpu=0, ids=None) == STATE and "not committed" in b.last_error().decode()
    assert _call(b, sc, _params(), _adaptive(), ngpu=64, ids=(0,) * 64) == STATE
    assert _call(b, sc, _params(), _adaptive(), win=(0, 0, W, H)) == STATE     # the whole frame is a window


# 5. the state: (what is broken, header index or (record field, value), the word the message must hold)
STATE_BREAKS = [("magic", 0, "magic"), ("version", 1, "version"), ("width", 2, "width"), ("height", 3, "height"), ("pass_spp", 4, "pass_spp"),
                ("spp_chunk", 5, "spp_chunk"), ("seed low", 10, "seed"), ("background b", 15, "background"), ("lookfrom x", 16, "lookfrom"),
                ("close_time", 30, "close_time"),
                ("n NaN", ("n", float("nan")), "n is not a finite integer"), ("n inf", ("n", float("inf")), "n is not a finite integer"),
                ("n 0 beside a k", ("n", 0.0), "n is 0 but the record is not empty"),
                ("n B / 2", ("n", 32.0), "below pass_spp"), ("n B + 1", ("n", 65.0), "multiple of pass_spp"),
                ("n cap + B", ("n", 192.0), "the state holds more samples than the cap"), ("k wrong", ("k", 15.0), "k is not"),
                ("k NaN", ("k", float("nan")), "k is not a finite integer"), ("k for two passes", ("k", 32.0), "k is not")]


@pytest.mark.parametrize("name,what,msg", STATE_BREAKS, ids=[x[0] for x in STATE_BREAKS])
def test_a_broken_state_is_refused_before_the_scene_is_looked_at(name, what, msg):
    b = library.product()
    sc = S.Scene(b)
    p, a, cam = _params(spp_chunk=4), _adaptive(), camera()
    st = _break(_state(p, a, cam), what)
    for scene in (True, False):
        assert _call(b, sc, p, a, state=st, scene=scene) == INVALID, name
        err = b.last_error().decode()
        assert msg in err and NAME in err and "not committed" not in err, (name, err)


def test_empty_records_are_accepted_here_and_only_here():
    """A state whose records are all zero, and one with some zero records among full ones, reach validate(); a record with n == 0 and anything else
    nonzero — a sum, a mean, a k, an M2, the pad — is refused; and rttnw_render_adaptive_resume refuses the all-zero state as it always did."""
    b = library.product()
    sc = S.Scene(b)
    p, a, cam = _params(spp_chunk=4), _adaptive(), camera()
    empty = _state(p, a, cam, n=0, k=0)
    assert not empty[64:].any()
    for call in ({}, {"ngpu": 0, "ids": None}):
        assert _call(b, sc, p, a, state=empty, **call) == STATE and "not committed" in b.last_error().decode()
        assert _call(b, sc, p, a, state=empty, scene=False, **call) == INVALID and "NULL" in b.last_error().decode()
    mixed = _state(p, a, cam)
    mixed[64:].reshape(-1, 12)[7:40] = 0.0
    assert _call(b, sc, p, a, state=mixed) == STATE and "not committed" in b.last_error().decode()
    for field in ("sum", "mu", "k", "m2", "pad"):
        bad = _break(empty, (field, 0.25 if field != "k" else 16.0))
        assert _call(b, sc, p, a, state=bad) == INVALID, field
        err = b.last_error().decode()
        assert "render_adaptive_region: state_in: a record's n is 0 but the record is not empty" in err and "(pixel 5)" in err, (field, err)
    for st in (empty, mixed):
        assert _call(b, sc, p, a, state=st, resume=True) == INVALID
        err = b.last_error().decode()
        assert err.startswith("render_adaptive_resume: state_in: a record's n is below pass_spp (pixel "), err


def test_refusals_come_in_the_stated_order():
    """A call that breaks two rules returns the earlier one's code and message."""
    b = library.product()
    sc = S.Scene(b)
    err = lambda: b.last_error().decode()
    p, a, cam = _params(spp_chunk=4), _adaptive(), camera()
    good = _state(p, a, cam)
    bad = _break(good, 0)
    off = (3, 5, W + 1, 11)
    # 1 before 2
    assert _call(b, sc, None, _adaptive(), win=(4, 4, 4, 4)) == INVALID and "NULL" in err()
    assert _call(b, sc, _params(), None, win=off) == INVALID and "NULL" in err()
    # 2 before 3
    assert _call(b, sc, _params(), _adaptive(), win=off, ngpu=65, ids=(0,) * 65) == INVALID and "window" in err()
    assert _call(b, sc, _params(), _adaptive(), win=off, ids=None) == INVALID and "window" in err()
    # 3 before 4
    assert _call(b, sc, _params(), _adaptive(pass_spp=0), ngpu=65, ids=(0,) * 65) == INVALID and "ngpu" in err()
    assert _call(b, sc, _params(collect_counters=1), _adaptive(), ids=None) == INVALID and "device_ids" in err()
    assert _call(b, sc, _params(spp=96), _adaptive(), ngpu=0, ids=(0,)) == INVALID and "device_ids" in err()
    # inside 4: the single call's order — pass_spp, the cap, the tolerances, reserved0, tile_world (ngpu == 0), collect_counters
    assert _call(b, sc, _params(spp=96), _adaptive(pass_spp=0)) == INVALID and "pass_spp is 0" in err()
    assert _call(b, sc, _params(spp=96), _adaptive(rel_error=-1.0)) == INVALID and "multiple of pass_spp" in err()
    assert _call(b, sc, _params(), _adaptive(rel_error=-1.0, reserved0=1)) == INVALID and "rel_error" in err()
    assert _call(b, sc, _params(collect_counters=1), _adaptive(reserved0=1)) == INVALID and "reserved0" in err()
    assert _call(b, sc, _params(collect_counters=1, tile_world=2), _adaptive(), ngpu=0, ids=None) == INVALID and "tile_world" in err()
    # 4 before 5: a bad state is not looked at while the adaptive arguments are wrong
    assert _call(b, sc, _params(collect_counters=1), _adaptive(), state=bad) == UNSUPPORTED and "collect_counters" in err()
    assert _call(b, sc, _params(), _adaptive(reserved0=1), state=bad) == INVALID and "reserved0" in err()
    # inside 5: magic, version, the header in its order, then the records
    assert _call(b, sc, p, a, state=_break(bad, 1)) == INVALID and "magic" in err()
    assert _call(b, sc, p, a, state=_break(_break(good, 1), 2)) == INVALID and "version" in err()
    assert _call(b, sc, p, a, state=_break(_break(good, 30), ("n", 0.0))) == INVALID and "close_time" in err()
    # 5 before 6: the state before a bad precision, a NULL or uncommitted scene
    pp = _params(precision=9, spp_chunk=4)
    assert _call(b, sc, pp, a, state=_break(_state(pp, a, cam), ("n", 65.0)), scene=False) == INVALID and "multiple of pass_spp" in err()
    assert _call(b, sc, p, a, state=bad, scene=False) == INVALID and "magic" in err()
    # 6 before 7: a device id nobody has is not looked at while the scene is not committed
    assert _call(b, sc, p, a, ids=(0, 1 << 20), state=good) == STATE and "not committed" in err()
    assert _call(b, sc, p, a, ids=(-1, 0), scene=False) == INVALID and "NULL" in err()


@pytest.mark.parametrize("argv,msg", [
    (["7", "--refine", "0,0,8,8"], "--refine needs --noise"),
    (["7", "--refine", "0,0,8,8", "--resume", "state.npy"], "--refine needs --noise"),
    (["7", "--noise", "0.1", "--refine", "0,0,8,8", "--window", "0,0,8,8"], "--refine does not combine with --window"),
    (["7", "--noise", "0.1", "--refine", "0,0,8,8", "--passes", "2"], "--refine does not combine with --passes"),
    (["7", "--noise", "0.1", "--refine", "0,0,8,8", "--features", "f"], "--refine does not combine with --features"),
    (["7", "--noise", "0.1", "--refine", "0,0,8,8", "--denoise"], "--refine does not combine with --denoise"),
    (["7", "--noise", "0.1", "--refine", "8,0,8,8", "--save-state", "state.npy"], "--refine wants X0,Y0,X1,Y1"),
])
def test_cli_refuses_before_any_scene_is_built(argv, msg, tmp_path):
    cli_refuses(argv, msg, tmp_path, must_not_exist=("state.npy", "f_albedo.png"))
