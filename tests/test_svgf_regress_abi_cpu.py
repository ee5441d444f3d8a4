"""rttnw_svgf_set_regress, rttnw_svgf_push_halves and rttnw_svgf_halves without a GPU: the exports exist and are declared alike in the header,
the ctypes binding and the Rust binding, with no new struct and no version bump; the header states the contract and points the two blocks whose
scope it closes at it; every refusal that needs no handle comes before the device is touched, in the order the header lists them — the handle
is checked last, which is what lets a NULL handle show the order —, with a message that names the call; the shared checker refuses for
rttnw_denoise_regress what it refused before; the Python driver and the command line refuse what they must before the library is called.
(tests/test_svgf_regress_cpu.py has the arithmetic, tests/test_gpu_svgf_regress.py what the device computes and the refusals that need a handle.)"""
import ctypes as C
import re

import numpy as np
import pytest

from abi_cases import FFI, HEADER, HEADER_TEXT, INVALID, camera, cli_refuses, declared_alike, exported
from rttnw_amd import abi, library, render

_CD = ("const double*", "*const f64", C.c_void_p)
_D = ("double*", "*mut f64", C.c_void_p)
_CAM = ("const rttnw_camera_desc*", "*const rttnw_camera_desc", C.POINTER(abi.CameraDesc))
_Q = ("rttnw_svgf*", "*mut rttnw_svgf", C.c_void_p)
_G = ("const rttnw_regress_params*", "*const rttnw_regress_params", C.POINTER(abi.Regress))
_OUT = ("const rttnw_svgf_out*", "*const rttnw_svgf_out", C.POINTER(abi.SvgfOut))
NAN = float("nan")


def test_exports_and_declarations():
    for name in ("svgf_set_regress", "svgf_push_halves", "svgf_halves"):
        exported(name)
        assert "rttnw_" + name in HEADER_TEXT.split("typedef struct rttnw_scene")[0], "the comment at RTTNW_ABI_VERSION says how a caller detects the function"
    declared_alike("svgf_set_regress", [("q",) + _Q, ("g",) + _G, ("variance_source", "uint32_t", "u32", C.c_uint32)])
    declared_alike("svgf_push_halves", [("q",) + _Q, ("cam",) + _CAM] + [(n,) + _CD for n in ("half_a", "half_b", "albedo", "normal", "depth", "alpha")] +
                   [("out",) + _OUT])
    declared_alike("svgf_halves", [("q",) + _Q] + [(n,) + _D for n in ("out_acc_a", "out_acc_b", "out_filtered_a", "out_filtered_b", "out_fit")])
    assert render.HALVES_ARRAYS == ("acc_a", "acc_b", "filtered_a", "filtered_b", "fit")


def test_no_new_struct_and_the_old_ones_unchanged():
    assert not re.search(r"pub struct rttnw_\w*(halves|svgf_regress)\w*\s*\{", FFI)
    assert C.sizeof(abi.Svgf) == 104 and C.sizeof(abi.SvgfOut) == 8 * 16 and C.sizeof(abi.Regress) == 40
    block = HEADER.split("int rttnw_svgf_samples(")[1].split("int rttnw_svgf_halves(")[0]
    assert "struct" not in block


def test_the_header_states_the_contract():
    contract = HEADER_TEXT.split("int rttnw_svgf_set_regress(")[0].split("int rttnw_svgf_samples(")[1]
    contract = re.sub(r"\n \*\s*", " ", contract)
    for phrase in ("The contract is a composition of the existing entry points, bit for bit", "the state gains Ha and Hb", "C = (a + b) * 0.5",
                   "this is raw_rgb", "giving c, ca, cb", "the \"was divided\" channels are C's", "The handle's step 1 on c, unchanged",
                   "equal bit for bit those of a plain handle (feedback 0, the same t, v and demodulate) pushed with C",
                   "prev_linear_rgb = Ha, prev_length = L", "Ab likewise from cb over Hb", "the four taps are computed once and carry four quantities",
                   "Without a state Aa = ca and Ab = cb", "there is no feedback",
                   "R = rttnw_denoise_regress(Aa, Ab, var_a, var_b, F.albedo, F.normal, F.depth, F.alpha, g)", "var_a = var_b = var + var, one sum",
                   "its variance is twice M1's", "both NULL, the filter's own pair variance", "g->demodulate must be 0",
                   "F.albedo is passed as a regressor, not as a divisor", "rttnw_denoise_nlm(Aa, Ab, var_a, var_b) bit for bit",
                   "linear_rgb = R.out_linear_rgb multiplied back on the channels step 0 divided", "accumulated_rgb = (Aa + Ab) * 0.5",
                   "filtered_variance_rgb = R.out_error_rgb", "history_rgb = M1", "Ca = rttnw_render(spp = p->spp / 2, sample_begin)",
                   "sample_begin + p->spp / 2", "p->spp must be even and at least 2", "stats sums the two traces", "every array is all 0",
                   "resets the history, as rttnw_svgf_reset does", "is a no-op and keeps the history", "frame calls still allocate nothing",
                   "a second packed trace buffer", "Ha and Hb as ping-pong pairs", "exclusive with feedback_iterations != 0, a clamp and sampling",
                   "everything rttnw_denoise_regress refuses for g, in its order; g->demodulate != 0; variance_source > 1; a NULL q (the handle is checked last)",
                   "rttnw_svgf_push refuses one", "after rttnw_svgf_push's own checks", "Out of scope", "rttnw_denoise_select as a stage",
                   "feeding the filtered halves back", "a sample-weighted blend", "a node-wide form", "the native rttnw program"):
        assert phrase in contract, phrase
    # the two blocks whose scope this closes point at it
    svgf = re.sub(r"\n \*\s*", " ", HEADER_TEXT.split("typedef struct rttnw_svgf rttnw_svgf;")[0])
    assert "now live below, at rttnw_svgf_set_regress" in svgf
    regress = re.sub(r"\n \*\s*", " ", HEADER_TEXT.split("struct rttnw_regress_params {")[0])
    assert "the SVGF handle (which now lives below, at rttnw_svgf_set_regress)" in regress


def _g(**kw):
    g = abi.Regress(search_radius=0, patch_radius=0, k=0.0, ridge=0.0, features=7, demodulate=0, reserved0=0, reserved1=0)
    for key, val in kw.items():
        setattr(g, key, val)
    return g


# rttnw_denoise_regress's refusals for g, in its order; then the stage's own; then the handle
SET_REFUSALS = [
    ("search_radius 17", {"search_radius": 17}, "g->search_radius"),
    ("patch_radius 5", {"patch_radius": 5}, "g->patch_radius"),
    ("negative k", {"k": -0.5}, "g->k"),
    ("NaN k", {"k": NAN}, "g->k"),
    ("features 8", {"features": 8}, "g->features"),
    ("negative ridge", {"ridge": -1e-3}, "g->ridge"),
    ("NaN ridge", {"ridge": NAN}, "g->ridge"),
    ("reserved0", {"reserved0": 1}, "g->reserved0"),
    ("reserved1", {"reserved1": 9}, "g->reserved0 and g->reserved1"),
    ("demodulate", {"demodulate": 1}, "g->demodulate must be 0"),
    ("variance_source 2", {"variance_source": 2}, "variance_source"),
    ("a NULL handle", {}, "q is NULL"),
]


def _set(b, **kw):
    source = kw.pop("variance_source", 0)
    return b.svgf_set_regress(None, C.byref(_g(**kw)), source)


@pytest.mark.parametrize("what,kw,msg", SET_REFUSALS, ids=[r[0] for r in SET_REFUSALS])
def test_set_regress_refuses_before_the_device(what, kw, msg):
    b = library.product()
    assert _set(b, **kw) == INVALID, what
    err = b.last_error().decode()
    assert err.startswith("svgf_set_regress:") and msg in err, (what, err)


def test_set_regress_refuses_in_the_order_the_header_lists():
    """Two faults per call: the earlier one of the table is the one reported."""
    b = library.product()
    faults = [(kw, msg) for what, kw, msg in SET_REFUSALS if kw and "NaN" not in what]
    seen = set()
    for i, (first, msg) in enumerate(faults):
        for later, _ in faults[i + 1:]:
            if set(first) & set(later):
                continue                                                    # (two values of one field are one fault)
            assert _set(b, **dict(first, **later)) == INVALID
            err = b.last_error().decode()
            assert err.startswith("svgf_set_regress:") and msg in err, (first, later, err)
            seen.add((tuple(first), tuple(later)))
    assert len(seen) >= 25
    # ... and the handle last: a NULL g on a NULL handle is refused for the handle, a good g too
    assert b.svgf_set_regress(None, None, 0) == INVALID and b.last_error().decode() == "svgf_set_regress: q is NULL"
    assert b.svgf_set_regress(None, None, 7) == INVALID and b.last_error().decode() == "svgf_set_regress: q is NULL"   # (no g: variance_source is not read)
    assert _set(b, features=0, variance_source=1) == INVALID and b.last_error().decode() == "svgf_set_regress: q is NULL"


def test_the_shared_checker_serves_denoise_regress_as_before():
    """The same texts under the other call's name, behind that call's own checks of its arrays."""
    b = library.product()
    a = np.ones(27)
    for _, kw, msg in SET_REFUSALS[:9]:
        g = _g(**kw)
        rc = b.denoise_regress(3, 3, a.ctypes.data, a.ctypes.data, None, None, a.ctypes.data, a.ctypes.data, a.ctypes.data, a.ctypes.data, C.byref(g),
                               None, None, None, None, None, None, None)
        assert rc == INVALID
        err = b.last_error().decode()
        assert err.startswith("denoise_regress:") and msg in err, err
    g = _g(search_radius=17)
    assert b.denoise_regress(3, 3, a.ctypes.data, a.ctypes.data, a.ctypes.data, None, None, None, None, None, C.byref(g), *[None] * 7) == INVALID
    assert "var_a and var_b go together" in b.last_error().decode()        # the arrays' checks still come before g's fields
    assert b.denoise_regress(3, 3, a.ctypes.data, a.ctypes.data, None, None, None, None, None, None, None, *[None] * 7) == INVALID
    assert b.last_error().decode() == "denoise_regress: g is NULL"


def _push_halves(b, drop=()):
    arr = {k: np.ones(36) for k in ("half_a", "half_b", "albedo", "normal", "depth", "alpha")}
    cam = camera()
    return b.svgf_push_halves(None, None if "cam" in drop else C.byref(cam), *[None if k in drop else arr[k].ctypes.data for k in arr], None)


PUSH_REFUSALS = [(("cam",), "cam is NULL"), (("half_a",), "half_a or half_b"), (("half_b",), "half_a or half_b"), (("albedo",), "albedo"),
                 (("normal",), "normal"), (("depth",), "depth"), (("alpha",), "alpha"), ((), "q is NULL")]


@pytest.mark.parametrize("drop,msg", PUSH_REFUSALS, ids=["-".join(d) or "handle" for d, _ in PUSH_REFUSALS])
def test_push_halves_refuses_before_the_device(drop, msg):
    """rttnw_svgf_push's checks, half_a and half_b where linear_rgb stood (out itself may be NULL: it is in every call here)."""
    b = library.product()
    assert _push_halves(b, drop) == INVALID
    err = b.last_error().decode()
    assert err.startswith("svgf_push_halves:") and msg in err, err


def test_push_halves_refuses_in_push_s_order():
    b = library.product()
    for i, (first, msg) in enumerate(PUSH_REFUSALS[:-1]):
        for later, _ in PUSH_REFUSALS[i + 1:]:
            assert _push_halves(b, first + later) == INVALID
            assert msg in b.last_error().decode(), (first, later, b.last_error().decode())


def test_halves_refuses_a_null_handle():
    b = library.product()
    out = np.zeros(36)
    for args in ([None] * 5, [out.ctypes.data] + [None] * 4, [None] * 4 + [out.ctypes.data]):
        assert b.svgf_halves(None, *args) == INVALID and b.last_error().decode() == "svgf_halves: q is NULL"


def test_the_python_driver_refuses_before_the_library_is_called():
    class NoLibrary(render.SvgfSequence):
        def __init__(self):                                                 # no handle: a call that reached the library would fail on it
            self.width, self.height, self.handle, self._b = 4, 3, C.c_void_p(), None
    seq = NoLibrary()
    for kw, name in (({"variance": "spatial"}, "variance"), ({"mask": 8}, "mask"), ({"mask": -1}, "mask"), ({"ridge": -1.0}, "ridge"), ({"ridge": NAN}, "ridge")):
        with pytest.raises(ValueError, match=name):
            seq.set_regress(**kw)
    with pytest.raises(ValueError, match="no output named"):
        seq.halves(want=("acc_c",))
    with pytest.raises(ValueError, match="a half is 3x4x3"):
        seq.push_halves(np.zeros((3, 4, 3)), np.zeros((3, 5, 3)), None, camera())
    p = abi.Params(width=8, height=8, spp=4)
    for kw, name in (({"spatial": "bilateral"}, "spatial"), ({"spatial": "nlm", "regress_variance": "none"}, "regress_variance"),
                     ({"spatial": "regress", "feedback": 1}, "does not combine"), ({"spatial": "nlm", "clamp": 1.0}, "does not combine"),
                     ({"spatial": "regress", "sampling": 2}, "does not combine")):
        with pytest.raises(ValueError, match=name):
            render.render_sequence_device(None, [], p, **kw)
    p.spp = 3
    with pytest.raises(ValueError, match="even"):
        render.render_sequence_device(None, [], p, spatial="regress")


@pytest.mark.parametrize("argv,msg", [
    (["7", "--orbit", "3", "--spatial", "regress"], "--spatial and --regress-variance need --svgf"),
    (["7", "--orbit", "3", "--regress-variance", "pair"], "--spatial and --regress-variance need --svgf"),
    (["7", "--orbit", "3", "--svgf", "--regress-variance", "pair"], "--regress-variance needs --spatial nlm or --spatial regress"),
    (["7", "--orbit", "3", "--svgf", "--spatial", "atrous", "--regress-variance", "pair"], "--regress-variance needs --spatial nlm or --spatial regress"),
    (["7", "--orbit", "3", "--svgf", "--spatial", "regress", "--feedback", "1"], "does not combine with --feedback, --clamp or --boost"),
    (["7", "--orbit", "3", "--svgf", "--spatial", "nlm", "--clamp", "1"], "does not combine with --feedback, --clamp or --boost"),
    (["7", "--orbit", "3", "--svgf", "--spatial", "nlm", "--boost", "2"], "does not combine with --feedback, --clamp or --boost"),
    (["7", "--orbit", "3", "--svgf", "--spatial", "regress", "--spp", "3"], "two halves"),
    (["7", "--orbit", "3", "--svgf", "--spatial", "regress", "--fit-map", "fit.png"], "--fit-map with --svgf names one file per frame"),
    (["7", "--orbit", "3", "--svgf", "--fit-map", "fit_%03d.png"], "--fit-map need --denoise-regress"),
])
def test_cli_refuses_before_any_scene_is_built(argv, msg, tmp_path):
    cli_refuses(argv, msg, tmp_path, must_not_exist=("frame_000.png",))
