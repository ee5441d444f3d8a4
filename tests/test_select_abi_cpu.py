"""rttnw_denoise_select without a GPU: the export exists and is declared alike in the header, the ctypes binding and the Rust binding;
rttnw_select_params has one layout in all three; every argument refusal comes before the device is touched, with a message that names the entry
point and the argument; a valid call without a device fails loudly; the Python driver and the command line refuse what they must before the
library is called.  (tests/test_select_cpu.py has the arithmetic, tests/test_gpu_select.py what the device computes.)"""
import ctypes as C
import re

import numpy as np
import pytest

from abi_cases import FFI, HEADER, HEADER_TEXT, INVALID, RUST_SCENE, cli_refuses, declared_alike, exported
from rttnw_amd import abi, library, render

_D, _U8, _CD = ("double*", "*mut f64", C.c_void_p), ("uint8_t*", "*mut u8", C.c_void_p), ("const double*", "*const f64", C.c_void_p)
ARGS = [("width", "uint32_t", "u32", C.c_uint32), ("height", "uint32_t", "u32", C.c_uint32), ("half_a",) + _CD, ("half_b",) + _CD, ("var_a",) + _CD,
        ("var_b",) + _CD, ("albedo",) + _CD, ("normal",) + _CD, ("depth",) + _CD, ("alpha",) + _CD,
        ("dn", "const rttnw_denoise_params*", "*const rttnw_denoise_params", C.POINTER(abi.Denoise)),
        ("nl", "const rttnw_nlm_params*", "*const rttnw_nlm_params", C.POINTER(abi.Nlm)),
        ("sel", "const rttnw_select_params*", "*const rttnw_select_params", C.POINTER(abi.Select)), ("out_linear_rgb",) + _D, ("out_rgba8",) + _U8,
        ("out_blend",) + _D, ("out_feature_rgb",) + _D, ("out_nlm_rgb",) + _D, ("out_error_rgb",) + _D,
        ("kernel_ms", "double*", "*mut f64", C.POINTER(C.c_double))]
HIP = -4


def test_export_and_declarations():
    exported("denoise_select")
    declared_alike("denoise_select", ARGS)
    assert "rttnw_denoise_select" in HEADER_TEXT.split("typedef struct rttnw_scene")[0], "the comment at RTTNW_ABI_VERSION says how a caller detects the function"
    assert "pub fn denoise_select(" in RUST_SCENE, "the crate's safe wrapper"


def test_params_layout_agrees_in_header_ctypes_and_rust():
    body = re.search(r"struct rttnw_select_params \{(.*?)\};", HEADER, flags=re.S).group(1)
    c_fields = [" ".join(d.split()) for d in body.split(";") if d.strip()]
    assert c_fields == ["uint32_t error_radius", "uint32_t blend_radius", "double margin", "uint32_t use_default_margin, reserved0"]
    assert re.search(r"typedef struct rttnw_select_params rttnw_select_params;", HEADER)      # the two-step form, like rttnw_nlm_params
    attrs, rs_body = re.search(r"((?:#\[[^\]]*\]\s*)+)pub struct rttnw_select_params\s*\{(.*?)\n\}", FFI, flags=re.S).groups()
    assert "repr(C)" in attrs
    fields = [("error_radius", "u32", C.c_uint32), ("blend_radius", "u32", C.c_uint32), ("margin", "f64", C.c_double),
              ("use_default_margin", "u32", C.c_uint32), ("reserved0", "u32", C.c_uint32)]
    assert re.findall(r"pub (\w+)\s*:\s*(\w+),", rs_body) == [(n, r) for n, r, _ in fields]
    assert list(abi.Select._fields_) == [(n, t) for n, _, t in fields]
    assert C.sizeof(abi.Select) == 24 and [getattr(abi.Select, n).offset for n, _, _ in fields] == [0, 4, 8, 16, 20]


def test_the_header_states_the_contract_the_three_implementations_share():
    contract = HEADER_TEXT.split("struct rttnw_select_params {")[0].split("int rttnw_denoise_nlm(", 1)[1]
    contract = re.sub(r"\n \*\s*", " ", contract)                       # the comment's line breaks are not part of its wording
    for phrase in ("bit for bit what that entry point returns", "out_half_a, out_half_b of rttnw_denoise_nlm", "1e-10 + (E_F + E_N)", "clamped",
                   "left to right", "top to bottom", "the product rounded once", "a NaN S compares false", "exactly 1.0",
                   "two products and one sum, not fused", "give the same bits", "leaves every output bit-identical", "use_default_margin != 0 takes 0.01",
                   "Out of scope"):
        assert phrase in contract, phrase


def _call(b, drop=(), width=4, height=3, dn=None, nl=None, **skw):
    n = max(width * height, 1) * 3
    arr = {k: np.zeros(n) for k in ("half_a", "half_b", "var_a", "var_b", "albedo", "normal", "depth", "alpha")}
    d = abi.Denoise(iterations=5, reserved0=0, sigma_luminance=0.0, sigma_normal=0.0, sigma_depth=0.0)
    q = abi.Nlm(search_radius=0, patch_radius=0, k=0.0, reserved0=0, reserved1=0)
    s = abi.Select(error_radius=0, blend_radius=0, margin=0.0, use_default_margin=0, reserved0=0)
    for params, kw in ((d, dn or {}), (q, nl or {}), (s, skw)):
        for key, v in kw.items():
            setattr(params, key, v)
    ptr = lambda k: None if k in drop else arr[k].ctypes.data
    byref = lambda k, params: None if k in drop else C.byref(params)
    return b.denoise_select(width, height, *[ptr(k) for k in ("half_a", "half_b", "var_a", "var_b", "albedo", "normal", "depth", "alpha")],
                            byref("dn", d), byref("nl", q), byref("sel", s), None, None, None, None, None, None, None)


@pytest.mark.parametrize("what,kw,msg", [
    ("NULL half_a", {"drop": ("half_a",)}, "half_a"),
    ("NULL half_b", {"drop": ("half_b",)}, "half_b"),
    ("NULL albedo", {"drop": ("albedo",)}, "albedo"),
    ("NULL normal", {"drop": ("normal",)}, "normal"),
    ("NULL depth", {"drop": ("depth",)}, "depth"),
    ("NULL alpha", {"drop": ("alpha",)}, "alpha"),
    ("NULL dn", {"drop": ("dn",)}, "dn"),
    ("NULL nl", {"drop": ("nl",)}, "nl"),
    ("NULL sel", {"drop": ("sel",)}, "sel is NULL"),
    ("var_a alone", {"drop": ("var_b",)}, "var_a and var_b"),
    ("var_b alone", {"drop": ("var_a",)}, "var_a and var_b"),
    ("width 0", {"width": 0}, "width * height"),
    ("height 0", {"height": 0}, "width * height"),
    ("iterations 9", {"dn": {"iterations": 9}}, "dn->iterations"),
    ("dn reserved0", {"dn": {"reserved0": 1}}, "dn->reserved0"),
    ("negative sigma", {"dn": {"sigma_depth": -1.0}}, "sigma"),
    ("NaN sigma", {"dn": {"sigma_luminance": float("nan")}}, "sigma"),
    ("search_radius 17", {"nl": {"search_radius": 17}}, "nl->search_radius"),
    ("patch_radius 5", {"nl": {"patch_radius": 5}}, "nl->patch_radius"),
    ("nl reserved0", {"nl": {"reserved0": 1}}, "nl->reserved0"),
    ("nl reserved1", {"nl": {"reserved1": 1}}, "nl->reserved1"),
    ("negative k", {"nl": {"k": -0.5}}, "nl->k"),
    ("NaN k", {"nl": {"k": float("nan")}}, "nl->k"),
    ("error_radius 17", {"error_radius": 17}, "sel->error_radius"),
    ("blend_radius 9", {"blend_radius": 9}, "sel->blend_radius"),
    ("margin 2.5", {"margin": 2.5}, "sel->margin"),
    ("margin -2.5", {"margin": -2.5}, "sel->margin"),
    ("NaN margin", {"margin": float("nan")}, "sel->margin"),
    ("sel reserved0", {"reserved0": 1}, "sel->reserved0"),
])
def test_refusals_come_before_the_device(what, kw, msg):
    b = library.product()
    assert _call(b, **kw) == INVALID, what
    err = b.last_error().decode()
    assert err.startswith("denoise_select:") and msg in err, (what, err)


@pytest.mark.skipif(library.product().device_count() > 0, reason="a GPU is present")
@pytest.mark.parametrize("kw", [{}, {"drop": ("var_a", "var_b")}, {"error_radius": 16, "blend_radius": 8, "margin": -2.0}, {"margin": 2.0},
                                {"use_default_margin": 1, "margin": float("nan")}, {"error_radius": 1, "blend_radius": 1, "dn": {"iterations": 0}}])
def test_a_valid_call_without_a_device_fails_loudly(kw):
    """(With use_default_margin set, margin is ignored: whatever it holds is not refused.)"""
    b = library.product()
    assert _call(b, **kw) == HIP
    assert "no CPU fallback" in b.last_error().decode() and "denoise_select" in b.last_error().decode()


def test_the_python_driver_refuses_before_the_library_is_called():
    img = np.zeros((4, 5, 3))
    f = {"albedo": img, "normal": img, "depth": np.zeros((4, 5)), "alpha": np.zeros((4, 5))}
    with pytest.raises(ValueError, match="both or neither"):
        render.denoise_select(img, img, f, var_a=img)
    with pytest.raises(ValueError, match="HxWx3"):
        render.denoise_select(img, np.zeros((4, 6, 3)), f)
    for margin in (2.5, -3.0, float("nan")):
        with pytest.raises(ValueError, match="margin"):
            render.denoise_select(img, img, f, margin=margin)


@pytest.mark.parametrize("argv,msg", [
    (["7", "--denoise-select", "--spp", "15"], "--denoise-select needs an even --spp"),
    (["7", "--denoise-select", "--spp", "1"], "--denoise-select needs an even --spp"),
    (["7", "--denoise-select", "--denoise"], "--denoise-select does not combine with --denoise"),
    (["7", "--denoise-select", "--denoise-nlm"], "--denoise-select does not combine with --denoise-nlm"),
    (["7", "--denoise-select", "--noise", "0.1"], "--denoise-select does not combine with --noise"),
    (["7", "--denoise-select", "--features", "f"], "--denoise-select does not combine with --features"),
    (["7", "--denoise-select", "--devices", "0,0"], "--denoise-select does not combine with --devices"),
    (["7", "--denoise-select", "--window", "0,0,8,8"], "--denoise-select does not combine with --window"),
    (["7", "--denoise-select", "--passes", "2"], "--denoise-select does not combine with --passes"),
    (["7", "--denoise-select", "--select-margin", "2.5"], "--select-margin must be -2 .. 2"),
    (["7", "--denoise-select", "--select-margin", "nan"], "--select-margin must be -2 .. 2"),
    (["7", "--denoise-select", "--denoise-iterations", "9"], "--denoise-iterations must be 0 .. 8"),
    (["7", "--denoise-select", "--nlm-search-radius", "17"], "--nlm-search-radius must be 0 .. 16"),
    (["7", "--blend-map", "b.png"], "--blend-map needs --denoise-select"),
])
def test_cli_refuses_before_any_scene_is_built(argv, msg, tmp_path):
    cli_refuses(argv, msg, tmp_path, must_not_exist=("b.png",))
