"""rttnw_denoise_nlm without a GPU: the export exists and is declared alike in the header, the ctypes binding and the Rust binding;
rttnw_nlm_params has one layout in all three; every argument refusal comes before the device is touched, with a message that names the entry
point and the argument; a valid call without a device fails loudly; the Python drivers and the command line refuse what they must before any
scene is built.  (tests/test_nlm_cpu.py has the arithmetic, tests/test_gpu_nlm.py what the device computes.)"""
import ctypes as C
import re

import numpy as np
import pytest

from abi_cases import FFI, HEADER, HEADER_TEXT, INVALID, RUST_SCENE, cli_refuses, declared_alike, exported
from rttnw_amd import abi, library, render
from rttnw_amd import scene as S

_D, _U8, _CD = ("double*", "*mut f64", C.c_void_p), ("uint8_t*", "*mut u8", C.c_void_p), ("const double*", "*const f64", C.c_void_p)
ARGS = [("width", "uint32_t", "u32", C.c_uint32), ("height", "uint32_t", "u32", C.c_uint32), ("half_a",) + _CD, ("half_b",) + _CD, ("var_a",) + _CD,
        ("var_b",) + _CD, ("d", "const rttnw_nlm_params*", "*const rttnw_nlm_params", C.POINTER(abi.Nlm)), ("out_linear_rgb",) + _D,
        ("out_rgba8",) + _U8, ("out_half_a",) + _D, ("out_half_b",) + _D, ("out_error_rgb",) + _D,
        ("kernel_ms", "double*", "*mut f64", C.POINTER(C.c_double))]
HIP = -4


def test_export_and_declarations():
    exported("denoise_nlm")
    declared_alike("denoise_nlm", ARGS)
    assert "rttnw_denoise_nlm" in HEADER_TEXT.split("typedef struct rttnw_scene")[0], "the comment at RTTNW_ABI_VERSION says how a caller detects the function"
    assert "pub fn denoise_nlm(" in RUST_SCENE, "the crate's safe wrapper"


def test_params_layout_agrees_in_header_ctypes_and_rust():
    body = re.search(r"struct rttnw_nlm_params \{(.*?)\};", HEADER, flags=re.S).group(1)
    c_fields = [" ".join(d.split()) for d in body.split(";") if d.strip()]
    assert c_fields == ["uint32_t search_radius", "uint32_t patch_radius", "double k", "uint32_t reserved0, reserved1"]
    assert re.search(r"typedef struct rttnw_nlm_params rttnw_nlm_params;", HEADER)          # the two-step form, like rttnw_denoise_params
    attrs, rs_body = re.search(r"((?:#\[[^\]]*\]\s*)+)pub struct rttnw_nlm_params\s*\{(.*?)\n\}", FFI, flags=re.S).groups()
    assert "repr(C)" in attrs
    fields = [("search_radius", "u32", C.c_uint32), ("patch_radius", "u32", C.c_uint32), ("k", "f64", C.c_double), ("reserved0", "u32", C.c_uint32),
              ("reserved1", "u32", C.c_uint32)]
    assert re.findall(r"pub (\w+)\s*:\s*(\w+),", rs_body) == [(n, r) for n, r, _ in fields]
    assert list(abi.Nlm._fields_) == [(n, t) for n, _, t in fields]
    assert C.sizeof(abi.Nlm) == 24 and [getattr(abi.Nlm, n).offset for n, _, _ in fields] == [0, 4, 8, 16, 20]


def test_the_header_states_the_contract_the_three_implementations_share():
    contract = HEADER_TEXT.split("struct rttnw_nlm_params {")[0].split("int rttnw_denoise(", 1)[1]
    for phrase in ("clamped", "row-major", "left to right", "top to bottom", "(3 * (2f + 1)^2)", "1e-10", "centre offset weighs exactly 1", "not special-cased",
                   "give the same bits", "Out of scope"):
        assert phrase in contract, phrase


def _call(b, drop=(), width=4, height=3, **dkw):
    n = max(width * height, 1) * 3
    arr = {k: np.zeros(n) for k in ("half_a", "half_b", "var_a", "var_b")}
    d = abi.Nlm(search_radius=0, patch_radius=0, k=0.0, reserved0=0, reserved1=0)
    for key, v in dkw.items():
        setattr(d, key, v)
    ptr = lambda k: None if k in drop else arr[k].ctypes.data
    return b.denoise_nlm(width, height, ptr("half_a"), ptr("half_b"), ptr("var_a"), ptr("var_b"), None if "d" in drop else C.byref(d), None, None, None,
                         None, None, None)


@pytest.mark.parametrize("what,kw,msg", [
    ("NULL half_a", {"drop": ("half_a",)}, "half_a"),
    ("NULL half_b", {"drop": ("half_b",)}, "half_b"),
    ("NULL d", {"drop": ("d",)}, "NULL"),
    ("var_a alone", {"drop": ("var_b",)}, "var_a and var_b"),
    ("var_b alone", {"drop": ("var_a",)}, "var_a and var_b"),
    ("width 0", {"width": 0}, "width * height"),
    ("height 0", {"height": 0}, "width * height"),
    ("search_radius 17", {"search_radius": 17}, "search_radius"),
    ("patch_radius 5", {"patch_radius": 5}, "patch_radius"),
    ("reserved0", {"reserved0": 1}, "reserved0"),
    ("reserved1", {"reserved1": 1}, "reserved1"),
    ("negative k", {"k": -0.5}, "d->k"),
    ("NaN k", {"k": float("nan")}, "d->k"),
])
def test_refusals_come_before_the_device(what, kw, msg):
    b = library.product()
    assert _call(b, **kw) == INVALID, what
    err = b.last_error().decode()
    assert err.startswith("denoise_nlm:") and msg in err, (what, err)


@pytest.mark.skipif(library.product().device_count() > 0, reason="a GPU is present")
@pytest.mark.parametrize("kw", [{}, {"drop": ("var_a", "var_b")}, {"search_radius": 16, "patch_radius": 4, "k": 2.0}, {"search_radius": 1, "patch_radius": 1}])
def test_a_valid_call_without_a_device_fails_loudly(kw):
    b = library.product()
    assert _call(b, **kw) == HIP
    assert "no CPU fallback" in b.last_error().decode() and "denoise_nlm" in b.last_error().decode()


def test_the_python_drivers_refuse_before_the_library_is_called():
    p = S.make_params(8, 8, 15)
    with pytest.raises(ValueError, match="even"):
        render.render_halves(None, None, p)
    p.spp = 0
    with pytest.raises(ValueError, match="even"):
        render.render_halves(None, None, p)
    img = np.zeros((4, 5, 3))
    with pytest.raises(ValueError, match="both or neither"):
        render.denoise_nlm(img, img, var_a=img)
    with pytest.raises(ValueError, match="HxWx3"):
        render.denoise_nlm(img, np.zeros((4, 6, 3)))


@pytest.mark.parametrize("argv,msg", [
    (["7", "--denoise-nlm", "--noise", "0.1"], "--denoise-nlm does not combine with --noise"),
    (["7", "--denoise-nlm", "--denoise"], "--denoise-nlm does not combine with --denoise"),
    (["7", "--denoise-nlm", "--features", "f"], "--denoise-nlm does not combine with --features"),
    (["7", "--denoise-nlm", "--devices", "0,0"], "--denoise-nlm does not combine with --devices"),
    (["7", "--denoise-nlm", "--window", "0,0,8,8"], "--denoise-nlm does not combine with --window"),
    (["7", "--denoise-nlm", "--passes", "2"], "--denoise-nlm does not combine with --passes"),
    (["7", "--denoise-nlm", "--nlm-search-radius", "17"], "--nlm-search-radius must be 0 .. 16"),
    (["7", "--denoise-nlm", "--nlm-patch-radius", "5"], "--nlm-patch-radius must be 0 .. 4"),
    (["7", "--denoise-nlm", "--nlm-k", "-1"], "--nlm-k must be at least 0"),
])
def test_cli_refuses_before_any_scene_is_built(argv, msg, tmp_path):
    cli_refuses(argv, msg, tmp_path)
