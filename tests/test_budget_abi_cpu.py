"""rttnw_budget_select and rttnw_render_adaptive_budget without a GPU: the exports exist and are declared alike in the header, the ctypes binding and
the Rust binding; rttnw_budget is 16 bytes in all three; every argument refusal comes before the device is touched — on a scene that was never
committed, and on no scene at all — in the order the header states, with a message that names the entry point and the field; and the command line
refuses --budget where it means nothing, before any scene is built.  (tests/test_gpu_budget_select.py and tests/test_gpu_adaptive_budget.py have
what the device computes.)"""
import ctypes as C
import re

import numpy as np
import pytest

from abi_cases import FFI, HEADER, HEADER_TEXT, INVALID, RUST_SCENE, STATE, UNSUPPORTED, camera, cli_refuses, declared_alike, exported, refused
from abi_cases import adaptive as _adaptive, break_state as _break, hand_made_state as _state, params as _params
from rttnw_amd import abi, library
from rttnw_amd import scene as S

# the argument lists, once: (name, C type, Rust type, ctypes type)
_D, _U8, _U32 = ("double*", "*mut f64", C.c_void_p), ("uint8_t*", "*mut u8", C.c_void_p), ("uint32_t*", "*mut u32", C.c_void_p)
_CD = ("const double*", "*const f64", C.c_void_p)
ARGS = {
    "budget_select": [("width", "uint32_t", "u32", C.c_uint32), ("height", "uint32_t", "u32", C.c_uint32), ("linear_rgb",) + _CD, ("stderr_rgb",) + _CD,
                      ("spp", "const uint32_t*", "*const u32", C.c_void_p), ("cap", "uint32_t", "u32", C.c_uint32),
                      ("rel_error", "double", "f64", C.c_double), ("abs_error", "double", "f64", C.c_double),
                      ("max_pixels", "uint64_t", "u64", C.c_uint64), ("out_mask",) + _U8, ("out_priority",) + _D,
                      ("out_selected", "uint64_t*", "*mut u64", C.POINTER(C.c_uint64)), ("kernel_ms", "double*", "*mut f64", C.POINTER(C.c_double))],
    "render_adaptive_budget": [("s", "rttnw_scene*", "*mut rttnw_scene", abi.scene_p),
                               ("cam", "const rttnw_camera_desc*", "*const rttnw_camera_desc", C.POINTER(abi.CameraDesc)),
                               ("p", "const rttnw_params*", "*const rttnw_params", C.POINTER(abi.Params)),
                               ("a", "const rttnw_adaptive*", "*const rttnw_adaptive", C.POINTER(abi.Adaptive)),
                               ("b", "const rttnw_budget*", "*const rttnw_budget", C.POINTER(abi.Budget)),
                               ("state_in",) + _CD, ("state_out",) + _D, ("out_linear_rgb",) + _D, ("out_rgba8",) + _U8, ("out_spp",) + _U32,
                               ("out_stderr_rgb",) + _D, ("stats", "rttnw_stats*", "*mut rttnw_stats", C.POINTER(abi.Stats))],
}


@pytest.mark.parametrize("name", ["budget_select", "render_adaptive_budget"])
def test_export_and_declarations(name):
    exported(name)
    declared_alike(name, ARGS[name])
    head = HEADER_TEXT.split("typedef struct rttnw_scene")[0]
    assert "rttnw_" + name in head and "by its symbol" in head, "the comment at RTTNW_ABI_VERSION says how a caller detects the function"
    assert "pub fn %s(" % name in RUST_SCENE, "the crate's safe wrapper"


def test_the_header_states_the_contract_and_what_is_out_of_scope():
    flat = lambda text: " ".join(text.replace("*", " ").split())          # the comment as prose: however it is wrapped
    contract = flat(HEADER_TEXT.split("struct rttnw_budget {")[0].split("int rttnw_budget_select(", 1)[1])
    assert "BIT-IDENTICAL" in contract and "rttnw_render_adaptive_region(window = the whole frame" in contract and "rel_error = abs_error = 0" in contract
    assert "rttnw_render_adaptive_resume(state_in = NULL)" in contract and "for any round_pixels" in contract
    assert "NOT promised to equal one call of N1 + N2" in contract
    assert "the one the adaptive render REPORTS" in contract and "not a division redone from the" in contract
    assert "refuses a state with a record above its cap" in contract and "set aside" in contract
    assert "Out of scope: a node-wide form (ngpu), windows and masks, and ranking by the filtered error" in contract
    assert "one small record in one copy" in contract
    select = flat(HEADER_TEXT.split("int rttnw_budget_select(", 1)[0].split("int rttnw_render_preview(", 1)[1])
    assert "NEVER READ" in select and "rho descending" in select and "(1, +inf]" in select and "integer atomics only" in select


def test_budget_layout_agrees_in_header_ctypes_and_rust():
    """rttnw_budget = a 64-bit word and two 32-bit words: 16 bytes, the same fields in the same order."""
    body = re.search(r"struct rttnw_budget \{(.*?)\};", HEADER, flags=re.S).group(1)
    c_fields = [tuple(" ".join(d.split()).rsplit(" ", 1)) for d in body.split(";") if d.strip()]
    assert c_fields == [("uint64_t", "samples"), ("uint32_t", "round_pixels"), ("uint32_t", "reserved0")]
    assert re.search(r"typedef struct rttnw_budget rttnw_budget;", HEADER)
    attrs, rs_body = re.search(r"((?:#\[[^\]]*\]\s*)+)pub struct rttnw_budget\s*\{(.*?)\n\}", FFI, flags=re.S).groups()
    assert "repr(C)" in attrs
    assert re.findall(r"pub (\w+)\s*:\s*(\w+),", rs_body) == [("samples", "u64"), ("round_pixels", "u32"), ("reserved0", "u32")]
    assert [(n, t) for n, t in abi.Budget._fields_] == [("samples", C.c_uint64), ("round_pixels", C.c_uint32), ("reserved0", C.c_uint32)]
    assert C.sizeof(abi.Budget) == 16
    assert abi.Budget.samples.offset == 0 and abi.Budget.round_pixels.offset == 8 and abi.Budget.reserved0.offset == 12


# ---------------------------------------------------------------- rttnw_budget_select's refusals

def _select_call(b, drop=(), width=4, height=3, cap=64, rel=0.05, ab=0.0):
    n = max(min(width * height, 64), 1)               # (a refused call reads none of them)
    arr = {"linear_rgb": np.zeros(n * 3), "stderr_rgb": np.zeros(n * 3), "spp": np.zeros(n, dtype=np.uint32)}
    ptr = lambda k: None if k in drop else arr[k].ctypes.data
    return b.budget_select(width, height, ptr("linear_rgb"), ptr("stderr_rgb"), ptr("spp"), cap, rel, ab, 5, None, None, None, None)


@pytest.mark.parametrize("what,kw,msg", [
    ("NULL linear_rgb", {"drop": ("linear_rgb",)}, "linear_rgb is NULL"),
    ("NULL stderr_rgb", {"drop": ("stderr_rgb",)}, "stderr_rgb is NULL"),
    ("NULL spp", {"drop": ("spp",)}, "spp is NULL"),
    ("empty width", {"width": 0}, "width * height"),
    ("empty height", {"height": 0}, "width * height"),
    ("cap 0", {"cap": 0}, "cap is 0"),
    ("negative rel", {"rel": -0.1}, "rel_error and abs_error"),
    ("NaN abs", {"ab": float("nan")}, "rel_error and abs_error"),
    ("both tolerances 0", {"rel": 0.0, "ab": 0.0}, "both 0"),
])
def test_select_refusals_come_before_the_device(what, kw, msg):
    b = library.product()
    assert _select_call(b, **kw) == INVALID, what
    err = b.last_error().decode()
    assert err.startswith("budget_select:") and msg in err, (what, err)


def test_select_refusals_come_in_the_stated_order():
    b = library.product()
    err = lambda: b.last_error().decode()
    assert _select_call(b, drop=("linear_rgb", "spp"), width=0) == INVALID and "linear_rgb" in err()
    assert _select_call(b, drop=("stderr_rgb", "spp"), width=0) == INVALID and "stderr_rgb" in err()
    assert _select_call(b, drop=("spp",), width=0, cap=0) == INVALID and "spp is NULL" in err()
    assert _select_call(b, width=0, cap=0) == INVALID and "width * height" in err()
    assert _select_call(b, cap=0, rel=-1.0) == INVALID and "cap is 0" in err()
    assert _select_call(b, rel=float("nan"), ab=0.0) == INVALID and "rel_error and abs_error" in err()
    assert _select_call(b, width=65536, height=65536) == UNSUPPORTED and "2^32 - 1" in err()      # the key holds the index in 32 bits


# ---------------------------------------------------------------- rttnw_render_adaptive_budget's refusals

NAME = "render_adaptive_budget"
def _budget(**kw):
    g = abi.Budget(samples=10000, round_pixels=0, reserved0=0)
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def _call(b, sc, p, a, g, scene=True, state=None):
    cam = camera()
    return b.render_adaptive_budget(sc.handle if scene else None, C.byref(cam), C.byref(p) if p is not None else None,
                                    C.byref(a) if a is not None else None, C.byref(g) if g is not None else None,
                                    None if state is None else state.ctypes.data, None, None, None, None, None, None)


@pytest.mark.parametrize("what,kw,adapt,budget,code,msg", [
    # 1. NULL p, a or b
    ("NULL p", None, {}, {}, INVALID, "NULL"),
    ("NULL a", {}, None, {}, INVALID, "NULL"),
    ("NULL b", {}, {}, None, INVALID, "NULL"),
    # 2. what rttnw_render_adaptive refuses among its own arguments, with its codes
    ("pass_spp 0", {}, {"pass_spp": 0}, {}, INVALID, "pass_spp is 0"),
    ("cap not a multiple", {"spp": 96}, {}, {}, INVALID, "multiple of pass_spp"),
    ("cap 0", {"spp": 0}, {}, {}, INVALID, "multiple of pass_spp"),
    ("negative rel", {}, {"rel_error": -0.1}, {}, INVALID, "rel_error and abs_error"),
    ("NaN abs", {}, {"abs_error": float("nan")}, {}, INVALID, "rel_error and abs_error"),
    ("a->reserved0", {}, {"reserved0": 1}, {}, INVALID, "reserved0"),
    ("tile_world", {"tile_world": 2}, {}, {}, INVALID, "tile_world"),
    ("counters", {"collect_counters": 1}, {}, {}, UNSUPPORTED, "collect_counters"),
    # 3. the budget's own field, then a tolerance of nothing
    ("b->reserved0", {}, {}, {"reserved0": 1}, INVALID, "b->reserved0"),
    ("both tolerances 0", {}, {"rel_error": 0.0, "abs_error": 0.0}, {}, INVALID, "both 0"),
    # 5. validate()
    ("bad precision", {"precision": 9}, {}, {}, None, "precision"),
    ("negative t_min", {"t_min": -1.0}, {}, {}, None, "t_min"),
    ("empty image", {"width": 0}, {}, {}, None, "empty image"),
])
def test_render_refusals_come_before_the_device(what, kw, adapt, budget, code, msg):
    b = library.product()
    sc = S.Scene(b)                                   # never committed: a device would be needed for that
    p = None if kw is None else _params(**kw)
    a = None if adapt is None else _adaptive(**adapt)
    g = None if budget is None else _budget(**budget)
    refused(b, lambda scene: _call(b, sc, p, a, g, scene=scene), code, msg, NAME)


def test_valid_budget_arguments_reach_validate():
    """Every value the contract allows — a budget of 0 and of 2^40 samples, rounds of 1 pixel and of more than the frame, one tolerance of 0 —
    passes the call's own checks, and so do a state of empty records and one of full ones."""
    b = library.product()
    sc = S.Scene(b)
    for budget in ({}, {"samples": 0}, {"samples": 1 << 40}, {"round_pixels": 1}, {"round_pixels": 1 << 31}):
        assert _call(b, sc, _params(), _adaptive(), _budget(**budget)) == STATE and "not committed" in b.last_error().decode(), budget
    assert _call(b, sc, _params(), _adaptive(rel_error=0.0, abs_error=0.01), _budget()) == STATE
    assert _call(b, sc, _params(spp=64), _adaptive(), _budget()) == STATE                          # cap == B
    p, a, cam = _params(spp_chunk=4), _adaptive(), camera()
    for st in (_state(p, a, cam), _state(p, a, cam, n=0, k=0)):
        assert _call(b, sc, p, a, _budget(), state=st) == STATE and "not committed" in b.last_error().decode()
        assert _call(b, sc, p, a, _budget(), state=st, scene=False) == INVALID and "NULL" in b.last_error().decode()


# 4. the state: (what is broken, header index or (record field, value), the word the message must hold)
STATE_BREAKS = [("magic", 0, "magic"), ("version", 1, "version"), ("width", 2, "width"), ("pass_spp", 4, "pass_spp"), ("close_time", 30, "close_time"),
                ("n NaN", ("n", float("nan")), "n is not a finite integer"), ("n 0 beside a k", ("n", 0.0), "n is 0 but the record is not empty"),
                ("n B + 1", ("n", 65.0), "multiple of pass_spp"), ("n cap + B", ("n", 192.0), "the state holds more samples than the cap"),
                ("k wrong", ("k", 15.0), "k is not")]


@pytest.mark.parametrize("name,what,msg", STATE_BREAKS, ids=[x[0] for x in STATE_BREAKS])
def test_a_broken_state_is_refused_before_the_scene_is_looked_at(name, what, msg):
    b = library.product()
    sc = S.Scene(b)
    p, a, cam = _params(spp_chunk=4), _adaptive(), camera()
    st = _break(_state(p, a, cam), what)
    for scene in (True, False):
        assert _call(b, sc, p, a, _budget(), state=st, scene=scene) == INVALID, name
        err = b.last_error().decode()
        assert err.startswith("render_adaptive_budget: state_in: ") and msg in err and "not committed" not in err, (name, err)


def test_render_refusals_come_in_the_stated_order():
    """A call that breaks two rules returns the earlier one's code and message."""
    b = library.product()
    sc = S.Scene(b)
    err = lambda: b.last_error().decode()
    p, a, cam = _params(spp_chunk=4), _adaptive(), camera()
    bad = _break(_state(p, a, cam), 0)
    # 1 before 2 and 3
    assert _call(b, sc, None, _adaptive(pass_spp=0), _budget(reserved0=1)) == INVALID and "NULL" in err()
    assert _call(b, sc, _params(spp=96), None, _budget()) == INVALID and "NULL" in err()
    assert _call(b, sc, _params(spp=96), _adaptive(), None) == INVALID and "NULL" in err()
    # inside 2: the single call's order — pass_spp, the cap, the tolerances, reserved0, tile_world, collect_counters
    assert _call(b, sc, _params(spp=96), _adaptive(pass_spp=0), _budget()) == INVALID and "pass_spp is 0" in err()
    assert _call(b, sc, _params(spp=96), _adaptive(rel_error=-1.0), _budget()) == INVALID and "multiple of pass_spp" in err()
    assert _call(b, sc, _params(), _adaptive(rel_error=-1.0, reserved0=1), _budget()) == INVALID and "rel_error" in err()
    assert _call(b, sc, _params(tile_world=2), _adaptive(reserved0=1), _budget()) == INVALID and "reserved0" in err() and "b->" not in err()
    assert _call(b, sc, _params(collect_counters=1, tile_world=2), _adaptive(), _budget()) == INVALID and "tile_world" in err()
    # 2 before 3
    assert _call(b, sc, _params(collect_counters=1), _adaptive(), _budget(reserved0=1)) == UNSUPPORTED and "collect_counters" in err()
    assert _call(b, sc, _params(tile_world=2), _adaptive(rel_error=0.0), _budget()) == INVALID and "tile_world" in err()
    # inside 3: b->reserved0, then the tolerances of nothing
    assert _call(b, sc, _params(), _adaptive(rel_error=0.0), _budget(reserved0=1)) == INVALID and "b->reserved0" in err()
    # 3 before 4: a bad state is not looked at while the budget's arguments are wrong
    assert _call(b, sc, p, a, _budget(reserved0=1), state=bad) == INVALID and "b->reserved0" in err()
    assert _call(b, sc, p, _adaptive(rel_error=0.0), _budget(), state=bad) == INVALID and "both 0" in err()
    # 4 before 5: the state before a bad precision, a NULL or uncommitted scene
    assert _call(b, sc, p, a, _budget(), state=bad, scene=False) == INVALID and "magic" in err()
    pp = _params(precision=9, spp_chunk=4)
    assert _call(b, sc, pp, a, _budget(), state=_break(_state(pp, a, cam), ("n", 65.0))) == INVALID and "multiple of pass_spp" in err()
    assert _call(b, sc, pp, a, _budget(), state=_state(pp, a, cam)) == STATE and "not committed" in err()


@pytest.mark.parametrize("argv,msg", [
    (["7", "--budget", "100000"], "--budget needs --noise"),
    (["7", "--budget", "100000", "--denoise"], "--budget needs --noise"),
    (["7", "--noise", "0.1", "--budget", "100000", "--preview", "2"], "--budget does not combine with --preview"),
    (["7", "--noise", "0.1", "--budget", "100000", "--guided"], "--budget does not combine with --guided"),
    (["7", "--noise", "0.1", "--budget", "100000", "--refine", "0,0,8,8"], "--budget does not combine with --refine"),
    (["7", "--noise", "0.1", "--budget", "100000", "--devices", "0,0"], "--budget does not combine with --devices"),
    (["7", "--noise", "0.1", "--budget", "100000", "--window", "0,0,8,8"], "--budget does not combine with --window"),
    (["7", "--noise", "0.1", "--budget", "100000", "--passes", "2"], "--budget does not combine with --passes"),
    (["7", "--noise", "0.1", "--budget", "-5"], "--budget must be at least 0"),
    (["7", "--noise", "0", "--budget", "100000"], "--budget needs a noise bound above 0"),
])
def test_cli_refuses_before_any_scene_is_built(argv, msg, tmp_path):
    cli_refuses(argv + ["--save-state", str(tmp_path / "saved.npy")], msg, tmp_path, must_not_exist=("saved.npy",))
