"""rttnw_denoise_regress without a GPU: the export exists and is declared alike in the header, the ctypes binding and the Rust binding;
rttnw_regress_params has one layout in all three; the header states the contract and leaves its neighbours' blocks alone; every argument refusal
comes before the device is touched, in the order the header lists them, with a message that names the entry point and the argument; a valid call
without a device fails loudly; the Python driver and the command line refuse what they must before the library is called.
(tests/test_regress_cpu.py has the arithmetic, tests/test_gpu_regress.py what the device computes.)"""
import ctypes as C
import re

import numpy as np
import pytest

from abi_cases import FFI, HEADER, HEADER_TEXT, INVALID, cli_refuses, declared_alike, exported
from rttnw_amd import abi, library, render
from rttnw_amd.__main__ import regress_mask

_D, _U8, _CD = ("double*", "*mut f64", C.c_void_p), ("uint8_t*", "*mut u8", C.c_void_p), ("const double*", "*const f64", C.c_void_p)
INPUTS = ("half_a", "half_b", "var_a", "var_b", "albedo", "normal", "depth", "alpha")
ARGS = ([("width", "uint32_t", "u32", C.c_uint32), ("height", "uint32_t", "u32", C.c_uint32)] + [(name,) + _CD for name in INPUTS] +
        [("g", "const rttnw_regress_params*", "*const rttnw_regress_params", C.POINTER(abi.Regress)), ("out_linear_rgb",) + _D, ("out_rgba8",) + _U8,
         ("out_half_a",) + _D, ("out_half_b",) + _D, ("out_error_rgb",) + _D, ("out_fit",) + _D,
         ("kernel_ms", "double*", "*mut f64", C.POINTER(C.c_double))])
FIELDS = [("search_radius", "u32", C.c_uint32), ("patch_radius", "u32", C.c_uint32), ("k", "f64", C.c_double), ("ridge", "f64", C.c_double),
          ("features", "u32", C.c_uint32), ("demodulate", "u32", C.c_uint32), ("reserved0", "u32", C.c_uint32), ("reserved1", "u32", C.c_uint32)]
HIP = -4
NAN = float("nan")


def test_export_and_declaration():
    exported("denoise_regress")
    assert "rttnw_denoise_regress" in HEADER_TEXT.split("typedef struct rttnw_scene")[0], "the comment at RTTNW_ABI_VERSION says how a caller detects the function"
    declared_alike("denoise_regress", ARGS)
    assert HEADER.index("int rttnw_denoise_select(") < HEADER.index("int rttnw_denoise_regress(") < HEADER.index("int rttnw_temporal_accumulate("), \
        "the new block stands after rttnw_denoise_select's"


def test_params_layout_agrees_in_header_ctypes_and_rust():
    body = re.search(r"struct rttnw_regress_params \{(.*?)\};", HEADER, flags=re.S).group(1)
    c_fields = [" ".join(d.split()) for d in body.split(";") if d.strip()]
    assert c_fields == ["uint32_t search_radius, patch_radius", "double k", "double ridge", "uint32_t features", "uint32_t demodulate",
                        "uint32_t reserved0, reserved1"]
    assert re.search(r"typedef struct rttnw_regress_params rttnw_regress_params;", HEADER)
    attrs, rs_body = re.search(r"((?:#\[[^\]]*\]\s*)+)pub struct rttnw_regress_params\s*\{(.*?)\n\}", FFI, flags=re.S).groups()
    assert "repr(C)" in attrs
    assert re.findall(r"pub (\w+)\s*:\s*(\w+),", rs_body) == [(n, r) for n, r, _ in FIELDS]
    assert list(abi.Regress._fields_) == [(n, t) for n, _, t in FIELDS]
    assert C.sizeof(abi.Regress) == 40 and [getattr(abi.Regress, n).offset for n, _, _ in FIELDS] == [0, 4, 8, 16, 24, 28, 32, 36]
    assert C.sizeof(abi.Nlm) == 24 and C.sizeof(abi.Select) == 24, "the neighbours' blocks keep their layout"


def test_the_header_states_the_contract():
    contract = HEADER_TEXT.split("struct rttnw_regress_params {")[0].split("int rttnw_denoise_select(", 1)[1]
    contract = re.sub(r"\n \*\s*", " ", contract)                       # the comment's line breaks are not part of its wording
    for phrase in ("Moon, Carr and Yoon", "Bitterli et al. 2016", "no weight depends on the noise it averages", "keeps only the intercept",
                   "no CPU fallback", "every output is optional", "every sum starts from 0.0 and adds its terms in the order", "give the same bits",
                   "alpha != 0 and a channel with albedo > 1e-3", "given variances by albedo * albedo",
                   "is formed from the demodulated halves", "multiplied by the centre's albedo in the same channels, before step 6",
                   "are exactly rttnw_denoise_nlm's", "row-major (oy outer, ox inner) and the centre weight is 1",
                   "or 0 when the centre's alpha == 0", "With m == 0 no feature array is read for that pixel and no candidate is dropped",
                   "a candidate whose clamped pixel has alpha == 0 is dropped: it enters no sum", "albedo r g b, normal x y z, depth",
                   "(z_q - z_p) / z_p with z = depth / alpha", "0, 1, 3, 4, 6 or 7", "s = s + w;  t_c = t_c + w * y_c",
                   "wx_i = w * x_i, formed once per candidate and component", "A_ij = A_ij + wx_i * x_j for j <= i", "C_ic = C_ic + wx_i * y_c",
                   "After the loop: A_ii = A_ii + ridge * s", "the features first, the constant eliminated last",
                   "acc = acc - L_jk * L_ik for k = 0 .. i-1 in order", "L_ji = acc / L_ii", "the pivot test acc > 0 must hold", "L_jj = sqrt(acc)",
                   "u_j = (b_j - sum_k L_jk u_k) / L_jj", "den = s - uu", "(t_c - uG_c) / den", "when den >= 0.5 is false", "this includes a NaN",
                   "Cauchy-Schwarz", "the zero-order value t_c / s, over the same kept candidates", "uu = uG = 0.0",
                   "a' uses w_B and regresses half a; b' uses w_A and regresses half b", "out_fit w*h holds 0.0, 1.0 or 2.0",
                   "every output of rttnw_denoise_nlm is reproduced bit for bit, and the four feature arrays may be NULL",
                   "swaps out_half_a with out_half_b", "within r + f + 1 pixels of it only",
                   "Non-finite inputs are not special-cased beyond the two tests of step 5", "features has no default: 0 is meaningful",
                   "naming denoise_regress", "a NULL g", "features > 7", "a negative or NaN ridge", "a non-zero reserved field",
                   "alpha whenever features != 0", "demodulate != 0 with a NULL albedo or alpha", "Out of scope", "a third candidate",
                   "prefiltering the features", "a second-order or per-channel-bandwidth fit", "the SVGF handle", "a node-wide form",
                   "the native rttnw program"):
        assert phrase in contract, phrase
    from regress_ref import DEFAULTS
    assert "ridge 0 = the library default, %s" % ("%.0e" % DEFAULTS["ridge"]).replace("e-0", "e-") in contract, "the header names the default the tests' reference uses"


def test_the_neighbours_blocks_are_as_they_were():
    """rttnw_denoise_nlm's and rttnw_denoise_select's blocks still name what they left out — the new block is where it went — and the ABI version
    did not move."""
    before = re.sub(r"\n \*\s*", " ", HEADER_TEXT.split("int rttnw_denoise_regress(")[0])
    assert "Out of scope: multiplying the first-hit normal and depth stops into the weight, albedo demodulation" in before
    assert "the native rttnw program, a third candidate filter" in before
    assert re.search(r"#define RTTNW_ABI_VERSION 3\b", HEADER)


def _call(b, drop=(), width=4, height=3, **gkw):
    n = max(width * height, 1) * 3
    arr = {name: np.ones(n) for name in INPUTS}
    g = abi.Regress(search_radius=0, patch_radius=0, k=0.0, ridge=0.0, features=7, demodulate=1, reserved0=0, reserved1=0)
    for key, val in gkw.items():
        setattr(g, key, val)
    ptr = lambda name: None if name in drop else arr[name].ctypes.data
    return b.denoise_regress(width, height, *[ptr(name) for name in INPUTS], None if "g" in drop else C.byref(g), *([None] * 7))


FEATURE_ARRAYS = ("albedo", "normal", "depth", "alpha")
# in the order the entry point checks: rttnw_denoise_nlm's list for the shared arguments, then g's own fields, then the arrays g asks for
REFUSALS = [
    ("NULL half_a", {"drop": ("half_a",)}, "half_a or half_b"),
    ("NULL half_b", {"drop": ("half_b",)}, "half_a or half_b"),
    ("NULL g", {"drop": ("g",)}, "g is NULL"),
    ("only var_a", {"drop": ("var_b",)}, "var_a and var_b go together"),
    ("only var_b", {"drop": ("var_a",)}, "var_a and var_b go together"),
    ("width 0", {"width": 0}, "width * height"),
    ("height 0", {"height": 0}, "width * height"),
    ("search_radius 17", {"search_radius": 17}, "g->search_radius"),
    ("patch_radius 5", {"patch_radius": 5}, "g->patch_radius"),
    ("negative k", {"k": -0.5}, "g->k"),
    ("NaN k", {"k": NAN}, "g->k"),
    ("features 8", {"features": 8}, "g->features"),
    ("features 2^31", {"features": 1 << 31}, "g->features"),
    ("negative ridge", {"ridge": -1e-3}, "g->ridge"),
    ("NaN ridge", {"ridge": NAN}, "g->ridge"),
    ("reserved0", {"reserved0": 1}, "g->reserved0"),
    ("reserved1", {"reserved1": 1}, "g->reserved0 and g->reserved1"),
    ("features 2 without alpha", {"features": 2, "demodulate": 0, "drop": ("alpha",)}, "alpha is NULL"),
    ("features 1 without albedo", {"features": 1, "demodulate": 0, "drop": ("albedo",)}, "albedo is NULL"),
    ("features 2 without normal", {"features": 2, "drop": ("normal",)}, "normal is NULL"),
    ("features 4 without depth", {"features": 4, "drop": ("depth",)}, "depth is NULL"),
    ("features 7 without depth", {"drop": ("depth",)}, "depth is NULL"),
    ("demodulate without albedo", {"features": 6, "drop": ("albedo",)}, "g->demodulate != 0 needs albedo and alpha"),
    ("demodulate without alpha", {"features": 0, "drop": ("alpha",)}, "g->demodulate != 0 needs albedo and alpha"),
    ("demodulate without any feature array", {"features": 0, "drop": FEATURE_ARRAYS}, "g->demodulate != 0 needs albedo and alpha"),
]


@pytest.mark.parametrize("what,kw,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_come_before_the_device(what, kw, msg):
    b = library.product()
    assert _call(b, **kw) == INVALID, what
    err = b.last_error().decode()
    assert err.startswith("denoise_regress:") and msg in err, (what, err)


def test_an_earlier_refusal_wins():
    """The order of the header's list."""
    b = library.product()
    for first, then in (({"drop": ("half_a", "g")}, "half_a or half_b"), ({"drop": ("g", "var_a")}, "g is NULL"), ({"drop": ("var_a",), "width": 0}, "var_a and var_b"),
                        ({"width": 0, "search_radius": 17}, "width * height"), ({"search_radius": 17, "patch_radius": 5}, "g->search_radius"),
                        ({"patch_radius": 5, "k": NAN}, "g->patch_radius"), ({"k": -1.0, "features": 8}, "g->k"), ({"features": 8, "ridge": NAN}, "g->features"),
                        ({"ridge": -1.0, "reserved0": 1}, "g->ridge"), ({"reserved1": 1, "drop": ("alpha",)}, "g->reserved0"),
                        ({"drop": ("alpha", "albedo", "normal", "depth")}, "alpha is NULL"), ({"drop": ("albedo", "normal")}, "albedo is NULL"),
                        ({"drop": ("normal", "depth")}, "normal is NULL"), ({"features": 4, "drop": ("depth", "albedo")}, "depth is NULL")):
        assert _call(b, **first) == INVALID
        assert then in b.last_error().decode(), (first, b.last_error().decode())


@pytest.mark.skipif(library.product().device_count() > 0, reason="a GPU is present")
@pytest.mark.parametrize("kw", [{}, {"drop": ("var_a", "var_b")}, {"features": 0, "demodulate": 0, "drop": FEATURE_ARRAYS},
                                {"features": 4, "demodulate": 0, "drop": ("albedo", "normal")}, {"features": 0, "drop": ("normal", "depth")},
                                {"search_radius": 16, "patch_radius": 4, "k": 2.0, "ridge": 1e-12, "features": 3}])
def test_a_valid_call_without_a_device_fails_loudly(kw):
    b = library.product()
    assert _call(b, **kw) == HIP
    assert "no CPU fallback" in b.last_error().decode() and "denoise_regress" in b.last_error().decode()


def test_the_python_driver_refuses_before_the_library_is_called():
    img, plane = np.zeros((4, 5, 3)), np.zeros((4, 5))
    f = {"albedo": img, "normal": img, "depth": plane, "alpha": plane}
    with pytest.raises(ValueError, match="both or neither"):
        render.denoise_regress(img, img, img, None, f)
    with pytest.raises(ValueError, match="HxWx3"):
        render.denoise_regress(img, np.zeros((4, 6, 3)), None, None, f)
    for kw, name in (({"mask": 8}, "mask"), ({"mask": -1}, "mask"), ({"ridge": -1.0}, "ridge"), ({"ridge": NAN}, "ridge")):
        with pytest.raises(ValueError, match=name):
            render.denoise_regress(img, img, None, None, f, **kw)
    for kw in ({}, {"mask": 0}, {"demodulate": False}):
        with pytest.raises(ValueError, match="need features"):
            render.denoise_regress(img, img, None, None, None, **kw)
    assert render.REGRESS_OUTPUTS == ("linear", "rgba8", "half_a", "half_b", "error", "fit")


def test_feature_letters():
    assert [regress_mask(t) for t in ("anz", "zna", "a", "n", "z", "az", "none")] == [7, 7, 1, 2, 4, 5, 0]
    assert [regress_mask(t) for t in ("", "x", "aa", "anzd", "None", "a,n")] == [None] * 6


@pytest.mark.parametrize("argv,msg", [
    (["7", "--spp", "15", "--denoise-regress"], "--denoise-regress needs an even --spp"),
    (["7", "--spp", "1", "--denoise-regress"], "--denoise-regress needs an even --spp"),
    (["7", "--spp", "16", "--denoise-regress", "--regress-features", "anx"], "--regress-features wants letters of a (albedo), n (normal), z (depth)"),
    (["7", "--spp", "16", "--denoise-regress", "--regress-features", ""], "--regress-features wants letters"),
    (["7", "--spp", "16", "--denoise-regress", "--ridge", "-1"], "--ridge must be at least 0"),
    (["7", "--spp", "16", "--denoise-regress", "--ridge", "nan"], "--ridge must be at least 0"),
    (["7", "--spp", "16", "--ridge", "0.1"], "need --denoise-regress"),
    (["7", "--spp", "16", "--denoise-nlm", "--fit-map", "fit.png"], "need --denoise-regress"),
    (["7", "--spp", "16", "--denoise-select", "--no-demodulate"], "need --denoise-regress"),
    (["7", "--spp", "16", "--denoise-regress", "--denoise-nlm"], "--denoise-regress does not combine with --denoise-nlm"),
    (["7", "--spp", "16", "--denoise-regress", "--noise", "0.05"], "--denoise-regress does not combine with --noise"),
    (["7", "--spp", "16", "--denoise-regress", "--nlm-search-radius", "17"], "--nlm-search-radius must be 0 .. 16"),
    (["7", "--orbit", "3", "--denoise-regress"], "--orbit does not combine with --denoise-regress"),
])
def test_cli_refuses_before_any_scene_is_built(argv, msg, tmp_path):
    cli_refuses(argv, msg, tmp_path, must_not_exist=("fit.png",))
