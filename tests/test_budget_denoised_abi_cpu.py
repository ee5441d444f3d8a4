"""rttnw_render_adaptive_budget_denoised without a GPU: the export exists and is declared alike in the header, the ctypes binding and the Rust
binding; every argument refusal comes before the device is touched — on a scene that was never committed, and on no scene at all — in the order
the header states, with a message that names the entry point and the field; and the command line refuses --guided-budget where it means nothing,
before any scene is built, while --budget --guided stays refused as it was.  (tests/test_gpu_adaptive_budget_denoised.py has what the device
computes.)"""
import ctypes as C

import pytest

from abi_cases import HEADER_TEXT, INVALID, RUST_SCENE, STATE, UNSUPPORTED, camera, cli_refuses, declared_alike, exported, refused
from abi_cases import adaptive as _adaptive, break_state as _break, hand_made_state as _state, params as _params
from rttnw_amd import abi, library
from rttnw_amd import scene as S

NAME = "render_adaptive_budget_denoised"
_D, _U8, _U32 = ("double*", "*mut f64", C.c_void_p), ("uint8_t*", "*mut u8", C.c_void_p), ("uint32_t*", "*mut u32", C.c_void_p)
_CD = ("const double*", "*const f64", C.c_void_p)
ARGS = [("s", "rttnw_scene*", "*mut rttnw_scene", abi.scene_p),
        ("cam", "const rttnw_camera_desc*", "*const rttnw_camera_desc", C.POINTER(abi.CameraDesc)),
        ("p", "const rttnw_params*", "*const rttnw_params", C.POINTER(abi.Params)),
        ("a", "const rttnw_adaptive*", "*const rttnw_adaptive", C.POINTER(abi.Adaptive)),
        ("b", "const rttnw_budget*", "*const rttnw_budget", C.POINTER(abi.Budget)),
        ("g", "const rttnw_guided*", "*const rttnw_guided", C.POINTER(abi.Guided)),
        ("state_in",) + _CD, ("state_out",) + _D, ("out_linear_rgb",) + _D, ("out_rgba8",) + _U8, ("out_valid",) + _U8, ("out_spp",) + _U32,
        ("out_stderr_rgb",) + _D, ("out_raw_linear_rgb",) + _D, ("out_raw_stderr_rgb",) + _D,
        ("stats", "rttnw_stats*", "*mut rttnw_stats", C.POINTER(abi.Stats))]


def test_export_and_declarations():
    exported(NAME)
    declared_alike(NAME, ARGS)
    head = HEADER_TEXT.split("typedef struct rttnw_scene")[0]
    assert "rttnw_" + NAME in head and "by its symbol" in head, "the comment at RTTNW_ABI_VERSION says how a caller detects the function"
    assert "pub fn %s(" % NAME in RUST_SCENE, "the crate's safe wrapper"


def test_the_header_states_the_contract_and_what_is_out_of_scope():
    flat = lambda text: " ".join(text.replace("*", " ").split())          # the comment as prose: however it is wrapped
    contract = flat(HEADER_TEXT.split("int rttnw_render_adaptive_budget_denoised(", 1)[0].split("int rttnw_render_adaptive_budget(", 1)[1])
    assert "BIT-IDENTICAL" in contract and "rttnw_reconstruct's out_linear_rgb, out_variance_rgb and out_valid" in contract
    assert "rttnw_render_adaptive_region(window = the whole frame" in contract and "rel_error = abs_error = 0" in contract
    assert "se_f = sqrt(var_f)" in contract and "whose OWN se is 0 in r, g and b" in contract and "min(round_pixels, remaining / B)" in contract
    assert "once more than the number of rounds" in contract and "state_in and state_out may be the same array" in contract
    assert "g->denoise.iterations == 0" in contract and "are rttnw_render_adaptive_budget's under the same arguments" in contract
    assert "NOT promised" in contract and "whose stops are sticky" in contract
    assert "Out of scope: a node-wide form (ngpu), and windows and masks." in contract


def _budget(**kw):
    g = abi.Budget(samples=10000, round_pixels=0, reserved0=0)
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def _guided(**kw):
    """iterations 3 and default sigmas; `kw` over rttnw_guided's own fields, and over its denoise parameters by their names."""
    g = abi.Guided(feature_spp=0, reserved0=0, denoise=abi.Denoise(iterations=3, reserved0=0, sigma_luminance=0.0, sigma_normal=0.0, sigma_depth=0.0))
    for k, v in kw.items():
        if k.startswith("denoise_"):
            setattr(g.denoise, k[len("denoise_"):], v)
        else:
            setattr(g, k, v)
    return g


def _call(b, sc, p, a, bg, g, scene=True, state=None):
    cam = camera()
    ref = lambda x: None if x is None else C.byref(x)
    return b.render_adaptive_budget_denoised(sc.handle if scene else None, C.byref(cam), ref(p), ref(a), ref(bg), ref(g),
                                             None if state is None else state.ctypes.data, None, None, None, None, None, None, None, None, None)


@pytest.mark.parametrize("what,kw,adapt,budget,guided,code,msg", [
    # 1. NULL p, a, b or g
    ("NULL p", None, {}, {}, {}, INVALID, "NULL"),
    ("NULL a", {}, None, {}, {}, INVALID, "NULL"),
    ("NULL b", {}, {}, None, {}, INVALID, "NULL"),
    ("NULL g", {}, {}, {}, None, INVALID, "NULL"),
    # 2. what rttnw_render_adaptive refuses among its own arguments, with its codes
    ("pass_spp 0", {}, {"pass_spp": 0}, {}, {}, INVALID, "pass_spp is 0"),
    ("cap not a multiple", {"spp": 96}, {}, {}, {}, INVALID, "multiple of pass_spp"),
    ("cap 0", {"spp": 0}, {}, {}, {}, INVALID, "multiple of pass_spp"),
    ("negative rel", {}, {"rel_error": -0.1}, {}, {}, INVALID, "rel_error and abs_error"),
    ("NaN abs", {}, {"abs_error": float("nan")}, {}, {}, INVALID, "rel_error and abs_error"),
    ("a->reserved0", {}, {"reserved0": 1}, {}, {}, INVALID, "reserved0"),
    ("tile_world", {"tile_world": 2}, {}, {}, {}, INVALID, "tile_world"),
    ("counters", {"collect_counters": 1}, {}, {}, {}, UNSUPPORTED, "collect_counters"),
    # 3. the budget's own field, then a tolerance of nothing
    ("b->reserved0", {}, {}, {"reserved0": 1}, {}, INVALID, "b->reserved0"),
    ("both tolerances 0", {}, {"rel_error": 0.0, "abs_error": 0.0}, {}, {}, INVALID, "both 0"),
    # 4. the filter's fields
    ("g->reserved0", {}, {}, {}, {"reserved0": 1}, INVALID, "g->reserved0"),
    ("iterations 9", {}, {}, {}, {"denoise_iterations": 9}, INVALID, "g->denoise.iterations"),
    ("g->denoise.reserved0", {}, {}, {}, {"denoise_reserved0": 1}, INVALID, "g->denoise.reserved0"),
    ("negative sigma", {}, {}, {}, {"denoise_sigma_normal": -1.0}, INVALID, "sigma"),
    ("NaN sigma", {}, {}, {}, {"denoise_sigma_depth": float("nan")}, INVALID, "sigma"),
    # 6. validate()
    ("bad precision", {"precision": 9}, {}, {}, {}, None, "precision"),
    ("negative t_min", {"t_min": -1.0}, {}, {}, {}, None, "t_min"),
    ("empty image", {"width": 0}, {}, {}, {}, None, "empty image"),
])
def test_refusals_come_before_the_device(what, kw, adapt, budget, guided, code, msg):
    b = library.product()
    sc = S.Scene(b)                                   # never committed: a device would be needed for that
    p = None if kw is None else _params(**kw)
    a = None if adapt is None else _adaptive(**adapt)
    bg = None if budget is None else _budget(**budget)
    g = None if guided is None else _guided(**guided)
    refused(b, lambda scene: _call(b, sc, p, a, bg, g, scene=scene), code, msg, NAME)


def test_valid_arguments_reach_validate():
    """Every value the contract allows — a budget of 0 and of 2^40 samples, rounds of 1 pixel and of more than the frame, one tolerance of 0, 0 and 8
    iterations, a feature_spp, positive sigmas — passes the call's own checks, and so do a state of empty records and one of full ones."""
    b = library.product()
    sc = S.Scene(b)
    for budget in ({}, {"samples": 0}, {"samples": 1 << 40}, {"round_pixels": 1}, {"round_pixels": 1 << 31}):
        assert _call(b, sc, _params(), _adaptive(), _budget(**budget), _guided()) == STATE and "not committed" in b.last_error().decode(), budget
    for guided in ({"denoise_iterations": 0}, {"denoise_iterations": 8}, {"feature_spp": 4}, {"denoise_sigma_luminance": 2.0, "denoise_sigma_depth": 0.5}):
        assert _call(b, sc, _params(), _adaptive(), _budget(), _guided(**guided)) == STATE and "not committed" in b.last_error().decode(), guided
    assert _call(b, sc, _params(), _adaptive(rel_error=0.0, abs_error=0.01), _budget(), _guided()) == STATE
    p, a, cam = _params(spp_chunk=4), _adaptive(), camera()
    for st in (_state(p, a, cam), _state(p, a, cam, n=0, k=0)):
        assert _call(b, sc, p, a, _budget(), _guided(), state=st) == STATE and "not committed" in b.last_error().decode()
        assert _call(b, sc, p, a, _budget(), _guided(), state=st, scene=False) == INVALID and "NULL" in b.last_error().decode()


# 5. the state: (what is broken, header index or (record field, value), the word the message must hold)
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
        assert _call(b, sc, p, a, _budget(), _guided(), state=st, scene=scene) == INVALID, name
        err = b.last_error().decode()
        assert err.startswith("render_adaptive_budget_denoised: state_in: ") and msg in err and "not committed" not in err, (name, err)


def test_refusals_come_in_the_stated_order():
    """A call that breaks two rules returns the earlier one's code and message."""
    b = library.product()
    sc = S.Scene(b)
    err = lambda: b.last_error().decode()
    p, a, cam = _params(spp_chunk=4), _adaptive(), camera()
    bad = _break(_state(p, a, cam), 0)
    # 1 before everything
    assert _call(b, sc, None, _adaptive(pass_spp=0), _budget(reserved0=1), _guided(reserved0=1)) == INVALID and "NULL" in err()
    assert _call(b, sc, _params(spp=96), _adaptive(), _budget(), None) == INVALID and "NULL" in err()
    # inside 2: the single call's order — pass_spp, the cap, the tolerances, reserved0, tile_world, collect_counters
    assert _call(b, sc, _params(spp=96), _adaptive(pass_spp=0), _budget(), _guided()) == INVALID and "pass_spp is 0" in err()
    assert _call(b, sc, _params(spp=96), _adaptive(rel_error=-1.0), _budget(), _guided()) == INVALID and "multiple of pass_spp" in err()
    assert _call(b, sc, _params(tile_world=2), _adaptive(reserved0=1), _budget(), _guided()) == INVALID and "reserved0" in err() and "->" not in err()
    assert _call(b, sc, _params(collect_counters=1, tile_world=2), _adaptive(), _budget(), _guided()) == INVALID and "tile_world" in err()
    # 2 before 3 and 4
    assert _call(b, sc, _params(collect_counters=1), _adaptive(), _budget(reserved0=1), _guided(reserved0=1)) == UNSUPPORTED and "collect_counters" in err()
    # inside 3: b->reserved0, then the tolerances of nothing; 3 before 4
    assert _call(b, sc, _params(), _adaptive(rel_error=0.0), _budget(reserved0=1), _guided(reserved0=1)) == INVALID and "b->reserved0" in err()
    assert _call(b, sc, _params(), _adaptive(rel_error=0.0), _budget(), _guided(reserved0=1)) == INVALID and "both 0" in err()
    # inside 4: g->reserved0, iterations, g->denoise.reserved0, the sigmas
    assert _call(b, sc, _params(), _adaptive(), _budget(), _guided(reserved0=1, denoise_iterations=9)) == INVALID and "g->reserved0" in err()
    assert _call(b, sc, _params(), _adaptive(), _budget(), _guided(denoise_iterations=9, denoise_reserved0=1)) == INVALID and "iterations" in err()
    assert _call(b, sc, _params(), _adaptive(), _budget(), _guided(denoise_reserved0=1, denoise_sigma_normal=-1.0)) == INVALID and "g->denoise.reserved0" in err()
    # 4 before 5: a bad state is not looked at while the filter's arguments are wrong
    assert _call(b, sc, p, a, _budget(), _guided(denoise_sigma_luminance=-1.0), state=bad) == INVALID and "sigma" in err() and "magic" not in err()
    # 5 before 6: the state before a bad precision, a NULL or uncommitted scene
    assert _call(b, sc, p, a, _budget(), _guided(), state=bad, scene=False) == INVALID and "magic" in err()
    pp = _params(precision=9, spp_chunk=4)
    assert _call(b, sc, pp, a, _budget(), _guided(), state=_break(_state(pp, a, cam), ("n", 65.0))) == INVALID and "multiple of pass_spp" in err()
    assert _call(b, sc, pp, a, _budget(), _guided(), state=_state(pp, a, cam)) == STATE and "not committed" in err()


GB = ["7", "--noise", "0.1", "--guided-budget", "100000"]


@pytest.mark.parametrize("argv,msg", [
    (["7", "--guided-budget", "100000"], "--guided-budget needs --noise"),
    (GB + ["--budget", "100000"], "--guided-budget does not combine with --budget"),
    (GB + ["--guided"], "--guided-budget does not combine with --guided"),
    (GB + ["--preview", "2"], "--guided-budget does not combine with --preview"),
    (GB + ["--refine", "0,0,8,8"], "--guided-budget does not combine with --refine"),
    (GB + ["--devices", "0,0"], "--guided-budget does not combine with --devices"),
    (GB + ["--window", "0,0,8,8"], "--guided-budget does not combine with --window"),
    (GB + ["--passes", "2"], "--guided-budget does not combine with --passes"),
    (["7", "--noise", "0.1", "--guided-budget", "-5"], "--guided-budget must be at least 0"),
    (["7", "--noise", "0", "--guided-budget", "100000"], "--guided-budget needs a noise bound above 0"),
    (GB + ["--denoise-iterations", "9"], "--denoise-iterations must be 0 .. 8"),
    # ... and the budgeted form still refuses the filter-guided one, in the words it always had
    (["7", "--noise", "0.1", "--budget", "100000", "--guided"], "--budget does not combine with --guided: it runs on one GPU, over the whole frame, on the raw noise"),
])
def test_cli_refuses_before_any_scene_is_built(argv, msg, tmp_path):
    cli_refuses(argv + ["--save-state", str(tmp_path / "saved.npy")], msg, tmp_path, must_not_exist=("saved.npy",))
