"""rttnw_render_region without a GPU: the export exists and is declared alike in the header, the ctypes binding and the Rust binding,
every argument refusal comes before the device is touched and in the order the header states, and the command line refuses a malformed
--window and its combination with --denoise before any render."""
import ctypes as C

import pytest

from abi_cases import HEADER_TEXT, INVALID, STATE, UNSUPPORTED, camera, cli_refuses, declared_alike, exported, params
from rttnw_amd import abi, library
from rttnw_amd import scene as S

# the argument list, once: (name, C type, Rust type, ctypes type)
ARGS = [("s", "rttnw_scene*", "*mut rttnw_scene", abi.scene_p),
        ("cam", "const rttnw_camera_desc*", "*const rttnw_camera_desc", C.POINTER(abi.CameraDesc)),
        ("p", "const rttnw_params*", "*const rttnw_params", C.POINTER(abi.Params)),
        ("x0", "uint32_t", "u32", C.c_uint32), ("y0", "uint32_t", "u32", C.c_uint32),
        ("x1", "uint32_t", "u32", C.c_uint32), ("y1", "uint32_t", "u32", C.c_uint32),
        ("mask", "const uint8_t*", "*const u8", C.c_void_p),
        ("out_linear_rgb", "double*", "*mut f64", C.c_void_p), ("out_rgba8", "uint8_t*", "*mut u8", C.c_void_p),
        ("stats", "rttnw_stats*", "*mut rttnw_stats", C.POINTER(abi.Stats))]


def test_export_and_declarations():
    exported("render_region")
    declared_alike("render_region", ARGS)
    assert "rttnw_render_region" in HEADER_TEXT.split("typedef struct rttnw_scene")[0], \
        "the comment at RTTNW_ABI_VERSION says how a caller detects the function"


def _region(b, sc, p, window=(2, 3, 10, 12), scene=True):
    cam = camera()
    return b.render_region(sc.handle if scene else None, C.byref(cam), C.byref(p) if p is not None else None, *window, None, None, None, None)


def _params(**kw):
    kw.setdefault("spp", 4)
    return params(**kw)


@pytest.mark.parametrize("what,window,kw,code,msg", [
    ("x0 == x1", (5, 3, 5, 12), {}, INVALID, "window"),
    ("y0 > y1", (2, 9, 10, 8), {}, INVALID, "window"),
    ("x1 == width + 1", (2, 3, 17, 12), {}, INVALID, "window"),
    ("y1 > height", (2, 3, 10, 40), {}, INVALID, "window"),
    ("reserved0", (2, 3, 10, 12), {"reserved0": 1}, INVALID, "reserved0"),
    ("tile_world", (2, 3, 10, 12), {"tile_world": 2}, INVALID, "tile_world"),
    ("counters", (2, 3, 10, 12), {"collect_counters": 1}, UNSUPPORTED, "collect_counters"),
])
def test_region_refusals_come_before_the_device(what, window, kw, code, msg):
    b = library.product()
    sc = S.Scene(b)                                   # never committed: a device would be needed for that
    assert _region(b, sc, _params(**kw), window) == code, what
    err = b.last_error().decode()
    assert err and msg in err, (what, err)
    assert _region(b, sc, _params(**kw), window, scene=False) == code, what      # ... nor any scene at all


def test_null_params_are_refused_first():
    b = library.product()
    sc = S.Scene(b)
    assert _region(b, sc, None) == INVALID and "NULL" in b.last_error().decode()
    assert _region(b, sc, None, window=(5, 5, 5, 5), scene=False) == INVALID and "NULL" in b.last_error().decode()


def test_refusals_come_in_the_stated_order():
    """A call that breaks two rules returns the earlier one's code and message."""
    b = library.product()
    sc = S.Scene(b)
    bad_window = (5, 3, 5, 12)
    assert _region(b, sc, _params(reserved0=1), bad_window) == INVALID and "window" in b.last_error().decode()
    assert _region(b, sc, _params(collect_counters=1), bad_window) == INVALID and "window" in b.last_error().decode()
    assert _region(b, sc, _params(reserved0=1, collect_counters=1)) == INVALID and "reserved0" in b.last_error().decode()
    assert _region(b, sc, _params(tile_world=2, collect_counters=1)) == INVALID and "tile_world" in b.last_error().decode()
    # collect_counters before what rttnw_render refuses: an empty spp, a bad precision, a NULL or uncommitted scene
    assert _region(b, sc, _params(collect_counters=1, spp=0)) == UNSUPPORTED and "collect_counters" in b.last_error().decode()
    assert _region(b, sc, _params(collect_counters=1, precision=9), scene=False) == UNSUPPORTED
    # ... and valid region arguments reach those checks
    assert _region(b, sc, _params()) == STATE and "not committed" in b.last_error().decode()
    assert _region(b, sc, _params(), window=(0, 0, 16, 16)) == STATE          # the whole frame is a window
    assert _region(b, sc, _params(), scene=False) == INVALID and "NULL" in b.last_error().decode()


@pytest.mark.parametrize("argv,msg", [
    (["7", "--window", "1,2,3"], "--window wants X0,Y0,X1,Y1"),
    (["7", "--window", "1,2,x,4"], "--window wants X0,Y0,X1,Y1"),
    (["7", "--window", "8,2,8,4"], "--window wants X0,Y0,X1,Y1"),
    (["7", "--window", "0,0,8,8", "--denoise"], "--window does not combine with --denoise"),
    (["7", "--window", "0,0,8,8", "--noise", "0.05"], "--window does not combine with --noise"),
    (["7", "--window", "0,0,8,8", "--features", "f"], "--window does not combine with --features"),
    (["7", "--window", "0,0,8,8", "--passes", "2"], "--window does not combine with --passes"),
])
def test_cli_refuses_before_any_render(argv, msg, tmp_path):
    cli_refuses(argv, msg, tmp_path)          # refused before the scene was even built
