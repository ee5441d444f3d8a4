"""rttnw_temporal_probe, rttnw_svgf_set_sampling and rttnw_svgf_samples without a GPU: the exports exist and are declared alike in the header, the
ctypes binding and the Rust binding; rttnw_sampling_params has one layout in all three; the header states the contract and leaves its neighbours'
blocks alone; every argument refusal comes before the device is touched, in the order the header lists them, with a message that names the entry
point and the argument; a valid call without a device fails loudly; the Python driver and the command line refuse what they must before the
library is called.  (tests/test_probe_cpu.py has the arithmetic, tests/test_gpu_probe.py and tests/test_gpu_svgf_sampling.py what the device
computes.)"""
import ctypes as C
import re

import numpy as np
import pytest

from abi_cases import FFI, HEADER, HEADER_TEXT, INVALID, camera, cli_refuses, declared_alike, exported
from rttnw_amd import abi, library, render

_D, _U8, _CD = ("double*", "*mut f64", C.c_void_p), ("uint8_t*", "*mut u8", C.c_void_p), ("const double*", "*const f64", C.c_void_p)
_CAM = ("const rttnw_camera_desc*", "*const rttnw_camera_desc", C.POINTER(abi.CameraDesc))
_Q = ("rttnw_svgf*", "*mut rttnw_svgf", C.c_void_p)
_A = ("const rttnw_sampling_params*", "*const rttnw_sampling_params", C.POINTER(abi.Sampling))
INPUTS = ("normal", "depth", "alpha", "prev_length", "prev_normal", "prev_depth", "prev_alpha")
ARGS = ([("width", "uint32_t", "u32", C.c_uint32), ("height", "uint32_t", "u32", C.c_uint32), ("cam",) + _CAM, ("prev_cam",) + _CAM] +
        [(name,) + _CD for name in INPUTS] +
        [("t", "const rttnw_temporal_params*", "*const rttnw_temporal_params", C.POINTER(abi.Temporal)), ("a",) + _A, ("out_length",) + _D,
         ("out_prev_xy",) + _D, ("out_multiplier",) + _U8, ("kernel_ms", "double*", "*mut f64", C.POINTER(C.c_double))])
HIP = -4
NAN, INF = float("nan"), float("inf")


def test_exports_and_declarations():
    for name in ("temporal_probe", "svgf_set_sampling", "svgf_samples"):
        exported(name)
        assert "rttnw_" + name in HEADER_TEXT.split("typedef struct rttnw_scene")[0], "the comment at RTTNW_ABI_VERSION says how a caller detects the function"
    declared_alike("temporal_probe", ARGS)
    declared_alike("svgf_set_sampling", [("q",) + _Q, ("a",) + _A])
    declared_alike("svgf_samples", [("q",) + _Q, ("out_spp", "uint32_t*", "*mut u32", C.c_void_p), ("out_length",) + _D])


def test_the_entry_point_takes_temporal_accumulates_arguments_without_the_colour():
    def names(fn):
        proto = re.search(r"\bint rttnw_%s\((.*?)\);" % fn, HEADER, flags=re.S).group(1)
        return [re.match(r".+?(\w+)$", a.strip()).group(1) for a in " ".join(proto.split()).split(",")]
    theirs, ours = names("temporal_accumulate"), names("temporal_probe")
    colour = ("linear_rgb", "variance_rgb", "prev_linear_rgb", "prev_variance_rgb")
    at = theirs.index("t") + 1
    assert ours[:ours.index("a")] == [n for n in theirs[:at] if n not in colour]
    assert ours[ours.index("a"):] == ["a", "out_length", "out_prev_xy", "out_multiplier", "kernel_ms"]
    assert HEADER.index("int rttnw_temporal_probe(") > HEADER.index("int rttnw_svgf_clipped("), "the new block stands after the clamp's"


def test_params_layout_agrees_in_header_ctypes_and_rust():
    body = re.search(r"struct rttnw_sampling_params \{(.*?)\};", HEADER, flags=re.S).group(1)
    c_fields = [" ".join(d.split()) for d in body.split(";") if d.strip()]
    assert c_fields == ["uint32_t boost", "uint32_t reserved0", "double fill"]
    assert re.search(r"typedef struct rttnw_sampling_params rttnw_sampling_params;", HEADER)
    attrs, rs_body = re.search(r"((?:#\[[^\]]*\]\s*)+)pub struct rttnw_sampling_params\s*\{(.*?)\n\}", FFI, flags=re.S).groups()
    assert "repr(C)" in attrs
    fields = [("boost", "u32", C.c_uint32), ("reserved0", "u32", C.c_uint32), ("fill", "f64", C.c_double)]
    assert re.findall(r"pub (\w+)\s*:\s*(\w+),", rs_body) == [(n, r) for n, r, _ in fields]
    assert list(abi.Sampling._fields_) == [(n, t) for n, _, t in fields]
    assert C.sizeof(abi.Sampling) == 16 and [getattr(abi.Sampling, n).offset for n, _, _ in fields] == [0, 4, 8]
    assert C.sizeof(abi.Svgf) == 104 and C.sizeof(abi.SvgfOut) == 8 * 16, "the handle's two blocks keep their layout"


def test_the_header_states_the_contract():
    contract = HEADER_TEXT.split("struct rttnw_sampling_params {")[0].split("int rttnw_svgf_clipped(", 1)[1]
    contract = re.sub(r"\n \*\s*", " ", contract)                       # the comment's line breaks are not part of its wording
    for phrase in ("it now lives here", "not its colour", "no CPU fallback", "the four taps in the order 00, 10, 01, 11",
                   "sw = sw + wt and sl = sl + wt * prev_length[tp]", "Where sw > 0, Lp = sl / sw", "Lp = 0.0 on every pass-through case",
                   "no history, alpha == 0, no place in the previous frame, or sw > 0 false", "out_length = Lp",
                   "out_prev_xy is rttnw_temporal_accumulate's", "k = floor(fill / (Lp + 1.0))", "the largest of 1, 2, 4, 8 that is <= min(k, boost)",
                   "m = 1 when k < 1", "m = 1 where this frame's alpha == 0", "Lp == 0 ? 1 : min(Lp + 1, max_history), bit for bit",
                   "the two out_prev_xy are equal bitwise, NaNs included", "give the same bits", "naming temporal_probe",
                   "a NULL a, a->boost not in {0, 1, 2, 4, 8}, a->reserved0 != 0, and a->fill that is NaN, infinite or in (0, 1)",
                   "takes effect from the next frame call", "keeps the history", "the handle is checked last", "allocates what it needs there and then",
                   "rttnw_svgf_push is unaffected", "The feature pass runs first", "so F keeps its bits",
                   "m = min(boost, largest power of two <= floor(fill)) on every hit pixel",
                   "rttnw_render(s, cam, p with spp = m(p) * p->spp, the same sample_begin), bit for bit", "rttnw_render_region under the mask {m == level}",
                   "Steps 0 to 5 of the handle's contract run on that C, unchanged, also with a clamp set",
                   "equals rttnw_svgf_push of that composed C and of F, in every output", "With boost = 1, or sampling never set",
                   "The plain pass traces EVERY pixel at p->spp", "are discarded", "an 8-byte copy", "the discarded samples included",
                   "out_spp w*h, m(p) * p->spp; out_length w*h, Lp", "Before any frame call out_spp is all 0 and out_length all 0",
                   "after a frame call without sampling out_spp is that call's p->spp everywhere and out_length all 0",
                   "[sample_begin, sample_begin + boost * spp)", "advances p->sample_begin by boost * p->spp a frame", "naming svgf_frame",
                   "the blend still weighs a frame as one frame",
                   "8, 4, 2, 2, 1, ... times spp", "Out of scope", "a sample-weighted history length", "dilating the multiplier map",
                   "a different rule for the first frame", "the variance, not only the length, as the driver", "a node-wide form",
                   "the native rttnw program"):
        assert phrase in contract, phrase


def test_the_neighbours_blocks_are_as_they_were():
    """The handle's block still names the gap, the new block says where it went, and the ABI version did not move."""
    before = re.sub(r"\n \*\s*", " ", HEADER_TEXT.split("int rttnw_svgf_frame(")[0])
    assert "adaptive sampling inside the sequence; colour clamping of the history" in before
    assert re.search(r"#define RTTNW_ABI_VERSION 3\b", HEADER)


def _call(b, drop=(), width=4, height=3, t=None, **akw):
    n = max(width * height, 1) * 3
    arr = {name: np.ones(n) for name in INPUTS}
    tp = abi.Temporal(max_history=0, reserved0=0, depth_tolerance=0.0, normal_min=0.0)
    for key, val in (t or {}).items():
        setattr(tp, key, val)
    ap = abi.Sampling(boost=0, reserved0=0, fill=0.0)
    for key, val in akw.items():
        setattr(ap, key, val)
    cam, prev_cam = camera(), camera()
    ptr = lambda name: None if name in drop else arr[name].ctypes.data
    return b.temporal_probe(width, height, None if "cam" in drop else C.byref(cam), None if "prev_cam" in drop else C.byref(prev_cam),
                            *[ptr(name) for name in INPUTS], None if "t" in drop else C.byref(tp), None if "a" in drop else C.byref(ap), *([None] * 4))


PREV = ("prev_length", "prev_normal", "prev_depth", "prev_alpha")
A_REFUSALS = [
    ("NULL a", {"drop": ("a",)}, "a is NULL"),
    ("boost 3", {"boost": 3}, "a->boost"),
    ("boost 16", {"boost": 16}, "a->boost"),
    ("boost 5", {"boost": 5}, "a->boost"),
    ("reserved0", {"reserved0": 1}, "a->reserved0"),
    ("NaN fill", {"fill": NAN}, "a->fill"),
    ("+inf fill", {"fill": INF}, "a->fill"),
    ("-inf fill", {"fill": -INF}, "a->fill"),
    ("fill 0.5", {"fill": 0.5}, "a->fill"),
    ("fill just under 1", {"fill": 1.0 - 2.0 ** -53}, "a->fill"),
    ("negative fill", {"fill": -8.0}, "a->fill"),
]
# in the order the entry point checks: rttnw_temporal_accumulate's list for the shared arguments (tests/test_temporal_abi_cpu.py), then a's
REFUSALS = [
    ("NULL cam", {"drop": ("cam",)}, "cam is NULL"),
    ("NULL normal", {"drop": ("normal",)}, "normal"),
    ("NULL depth", {"drop": ("depth",)}, "depth"),
    ("NULL alpha", {"drop": ("alpha",)}, "alpha"),
    ("NULL t", {"drop": ("t",)}, "t is NULL"),
    ("width 0", {"width": 0}, "width * height"),
    ("height 0", {"height": 0}, "width * height"),
] + [("without " + name, {"drop": (name,)}, "prev_* arrays go together") for name in PREV] + [
    ("only prev_length", {"drop": PREV[1:]}, "prev_* arrays go together"),
    ("only prev_alpha", {"drop": PREV[:3]}, "prev_* arrays go together"),
    ("a history without prev_cam", {"drop": ("prev_cam",)}, "prev_cam is NULL"),
    ("max_history 65536", {"t": {"max_history": 65536}}, "t->max_history"),
    ("t's reserved0", {"t": {"reserved0": 1}}, "t->reserved0"),
    ("negative depth_tolerance", {"t": {"depth_tolerance": -0.1}}, "t->depth_tolerance"),
    ("NaN depth_tolerance", {"t": {"depth_tolerance": NAN}}, "t->depth_tolerance"),
    ("normal_min 1.5", {"t": {"normal_min": 1.5}}, "t->normal_min"),
    ("NaN normal_min", {"t": {"normal_min": NAN}}, "t->normal_min"),
] + A_REFUSALS


@pytest.mark.parametrize("what,kw,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_come_before_the_device(what, kw, msg):
    b = library.product()
    assert _call(b, **kw) == INVALID, what
    err = b.last_error().decode()
    assert err.startswith("temporal_probe:") and msg in err, (what, err)


def test_an_earlier_refusal_wins():
    """The order of the header's list: rttnw_temporal_accumulate's, then a and its fields in the struct's order."""
    b = library.product()
    for first, then in (({"drop": ("cam", "a")}, "cam is NULL"), ({"drop": ("alpha", "t")}, "alpha"), ({"drop": ("t",), "width": 0}, "t is NULL"),
                        ({"width": 0, "drop": ("prev_alpha",)}, "width * height"), ({"drop": ("prev_alpha", "prev_cam", "a")}, "prev_* arrays"),
                        ({"drop": ("prev_cam",), "t": {"max_history": 65536}}, "prev_cam is NULL"),
                        ({"t": {"max_history": 65536, "reserved0": 1}, "drop": ("a",)}, "t->max_history"),
                        ({"t": {"normal_min": NAN}, "boost": 3}, "t->normal_min"), ({"boost": 3, "reserved0": 1}, "a->boost"),
                        ({"reserved0": 1, "fill": NAN}, "a->reserved0")):
        assert _call(b, **first) == INVALID
        assert then in b.last_error().decode(), (first, b.last_error().decode())


@pytest.mark.parametrize("what,kw,msg", A_REFUSALS[1:], ids=[r[0] for r in A_REFUSALS[1:]])
def test_set_sampling_refuses_the_same_block_before_it_looks_at_the_handle(what, kw, msg):
    b = library.product()
    ap = abi.Sampling(boost=0, reserved0=0, fill=0.0)
    for key, val in kw.items():
        setattr(ap, key, val)
    assert b.svgf_set_sampling(None, C.byref(ap)) == INVALID, what
    err = b.last_error().decode()
    assert err.startswith("svgf_set_sampling:") and msg in err, (what, err)


def test_the_handle_is_checked_last():
    b = library.product()
    for ap in (None, abi.Sampling(), abi.Sampling(boost=1, fill=1.0), abi.Sampling(boost=8, fill=1e300)):
        assert b.svgf_set_sampling(None, None if ap is None else C.byref(ap)) == INVALID
        assert b.last_error().decode() == "svgf_set_sampling: q is NULL"
    spp, length = np.zeros(12, dtype=np.uint32), np.zeros(12)
    for args in ((None, None), (spp.ctypes.data, length.ctypes.data)):
        assert b.svgf_samples(None, *args) == INVALID and b.last_error().decode() == "svgf_samples: q is NULL"


@pytest.mark.skipif(library.product().device_count() > 0, reason="a GPU is present")
@pytest.mark.parametrize("kw", [{}, {"drop": PREV + ("prev_cam",)}, {"drop": PREV}, {"boost": 1, "fill": 1.0}, {"boost": 8, "fill": 100.0},
                                {"boost": 2, "fill": 3.5, "t": {"max_history": 65535, "normal_min": -1.0}}])
def test_a_valid_call_without_a_device_fails_loudly(kw):
    b = library.product()
    assert _call(b, **kw) == HIP
    assert "no CPU fallback" in b.last_error().decode() and "temporal_probe" in b.last_error().decode()


def test_the_python_driver_refuses_before_the_library_is_called():
    img, plane = np.zeros((4, 5, 3)), np.zeros((4, 5))
    f = {"albedo": img, "normal": img, "depth": plane, "alpha": plane}
    cam = camera()
    history = {"length": plane, "features": f, "cam": cam}
    with pytest.raises(ValueError, match="HxW"):
        render.temporal_probe(dict(f, depth=img), cam)
    with pytest.raises(ValueError, match="it lacks length"):
        render.temporal_probe(f, cam, history=dict(history, length=None))
    with pytest.raises(ValueError, match="of one 5x4 frame"):
        render.temporal_probe(f, cam, history=dict(history, length=np.zeros((4, 6))))
    for kw, name in (({"max_history": 65536}, "max_history"), ({"depth_tolerance": NAN}, "depth_tolerance"), ({"normal_min": 2.0}, "normal_min"),
                     ({"boost": 3}, "boost"), ({"boost": 16}, "boost"), ({"boost": -1}, "boost"), ({"fill": 0.5}, "fill"), ({"fill": NAN}, "fill"),
                     ({"fill": INF}, "fill"), ({"fill": -1.0}, "fill")):
        with pytest.raises(ValueError, match=name):
            render.temporal_probe(f, cam, **kw)
    for sampling, name in ((3, "boost"), ((8, 0.5), "fill"), ((8, NAN), "fill"), ((8, 8.0, 1), "a boost or a pair")):
        with pytest.raises(ValueError, match=name):
            render.render_sequence_device(None, [], None, sampling=sampling)
    assert render.PROBE_OUTPUTS == ("length", "prev_xy", "multiplier")


@pytest.mark.parametrize("argv,msg", [
    (["7", "--boost", "8"], "--boost and --fill need --svgf"),
    (["7", "--orbit", "3", "--temporal-variance", "--boost", "8"], "--boost and --fill need --svgf"),
    (["7", "--orbit", "3", "--svgf", "--fill", "8"], "--fill needs --boost"),
    (["7", "--orbit", "3", "--svgf", "--boost", "3"], "--boost must be 1, 2, 4 or 8"),
    (["7", "--orbit", "3", "--svgf", "--boost", "16"], "--boost must be 1, 2, 4 or 8"),
    (["7", "--orbit", "3", "--svgf", "--boost", "8", "--fill", "0.5"], "--fill must be finite and at least 1"),
    (["7", "--orbit", "3", "--svgf", "--boost", "8", "--fill", "nan"], "--fill must be finite and at least 1"),
    (["7", "--orbit", "3", "--svgf", "--boost", "8", "--fill", "inf"], "--fill must be finite and at least 1"),
    (["7", "--orbit", "3", "--svgf", "--spp-map", "spp_%03d.png"], "--spp-map with --svgf needs --boost"),
    (["7", "--orbit", "3", "--svgf", "--boost", "8", "--spp-map", "spp.png"], "it needs a %d"),
    (["7", "--svgf", "--boost", "8"], "--svgf needs --orbit"),
])
def test_cli_refuses_before_any_scene_is_built(argv, msg, tmp_path):
    cli_refuses(argv, msg, tmp_path, must_not_exist=("frame_000.png", "spp_000.png", "spp.png"))
