"""The ORDER in which the image-filter entry points report their refusals, without a GPU: rttnw_denoise, rttnw_reconstruct, rttnw_denoise_nlm,
rttnw_denoise_select, rttnw_denoise_regress, rttnw_temporal_accumulate, rttnw_temporal_variance, rttnw_temporal_clamp, rttnw_temporal_probe,
rttnw_svgf_create, rttnw_svgf_push and rttnw_svgf_frame.  Every call has TWO faults, from neighbouring steps of the entry point's order, on a 4x3
image, and the earlier one is the one reported.  The order is the one include/rttnw_hip.h lists at each entry point — NULL pointers, the size, the
history, then the parameter blocks in the order of the signature, each block's fields in the order of its refusal list — and, where the header names
the faults without ranking them, the order the library has always had.  The entry points share one refusal function per parameter block
(rttnw_amd/csrc/feature_api.cpp): the single-fault tables of tests/test_*_abi_cpu.py say that each fault is refused, this file that sharing the
checks did not reorder them."""
import ctypes as C
import re

import numpy as np
import pytest

from abi_cases import HEADER, INVALID, UNSUPPORTED, camera, params
from rttnw_amd import abi, library

NAN = float("nan")
W, H = 4, 3
BLOCKS = {"rttnw_denoise_params": abi.Denoise, "rttnw_nlm_params": abi.Nlm, "rttnw_select_params": abi.Select, "rttnw_regress_params": abi.Regress,
          "rttnw_temporal_params": abi.Temporal, "rttnw_variance_params": abi.Variance, "rttnw_clamp_params": abi.Clamp,
          "rttnw_sampling_params": abi.Sampling, "rttnw_svgf_params": abi.Svgf}


def _prototype(name):
    proto = re.search(r"\bint rttnw_%s\((.*?)\);" % name, HEADER, flags=re.S).group(1)
    return [re.match(r"(.+?)\s*(\w+)$", a.strip()).groups() for a in " ".join(proto.split()).split(",")]


def _set(block, path, value):
    *outer, field = path.split(".")
    for name in outer:
        block = getattr(block, name)
    setattr(block, field, value)


def call(name, drop=(), **faults):
    """rttnw_<name> with valid arguments made from its prototype in the header — every input array there, every parameter block all zeros (the
    defaults), every output, the handle and the scene NULL — then `drop` (argument names) made NULL and `faults` laid over them: width, height, or
    {field: value} for a block, a dotted field reaching into a nested one."""
    keep, args = [], []
    for ctype, arg in _prototype(name):
        ctype = ctype.replace(" *", "*")
        const, base = ctype.startswith("const "), ctype.replace("const ", "").rstrip("*")
        if arg in drop:
            value = None
        elif arg in ("width", "height"):
            value = faults.get(arg, W if arg == "width" else H)
        elif base == "rttnw_camera_desc":
            value = camera()
        elif base == "rttnw_params":
            value = params(width=W, height=H, spp=4)
        elif base in BLOCKS:
            value = BLOCKS[base]()
        elif ctype == "rttnw_svgf**":
            value = C.c_void_p()
        elif const and base in ("double", "uint8_t"):
            value = np.ones(W * H * 3, dtype=np.float64 if base == "double" else np.uint8)
        else:
            value = None                                            # an output, the handle, the scene, the out block, the stats
        if isinstance(value, C.Structure) or isinstance(value, C.c_void_p):
            for path, v in (faults.get(arg) or {}).items():
                _set(value, path, v)
            keep.append(value)
            value = C.byref(value)
        elif isinstance(value, np.ndarray):
            keep.append(value)
            value = value.ctypes.data
        args.append(value)
    return getattr(library.product(), name)(*args)


# (entry point, the two faults, what the message must hold): the earlier fault's words
T_AND_BEFORE = [  # what the four history calls share, up to t's third field
    ({"drop": ("cam", "normal")}, "cam is NULL"),
    ({"drop": ("normal", "t")}, "NULL argument (normal, depth or alpha)"),
    ({"drop": ("t",), "width": 0}, "t is NULL"),
    ({"width": 0, "drop": ("prev_alpha",)}, "width * height"),
    ({"drop": ("prev_alpha", "prev_cam")}, "prev_* arrays go together"),
    ({"drop": ("prev_cam",), "t": {"max_history": 65536}}, "prev_cam is NULL"),
    ({"t": {"max_history": 65536, "reserved0": 1}}, "t->max_history"),
    ({"t": {"reserved0": 1, "depth_tolerance": -1.0}}, "t->reserved0"),
    ({"t": {"depth_tolerance": NAN, "normal_min": 2.0}}, "t->depth_tolerance"),
]
V_BLOCK = [
    ({"t": {"normal_min": NAN}, "drop": ("v",)}, "t->normal_min"),
    ({"v": {"min_temporal": 1, "radius": 5}}, "v->min_temporal"),
    ({"v": {"radius": 5, "reserved1": 1}}, "v->radius"),
    ({"v": {"reserved0": 1, "sigma_depth": NAN}}, "v->reserved0"),
]
DENOISE_BLOCK = [
    ({"width": 0, "d": {"iterations": 9}}, "width * height"),
    ({"d": {"iterations": 9, "reserved0": 1}}, "d->iterations: more than 8 iterations"),
    ({"d": {"reserved0": 1, "sigma_normal": -1.0}}, "d->reserved0"),
]
CASES = [("denoise", kw, msg) for kw, msg in [({"drop": ("d",), "width": 0}, "NULL argument")] + DENOISE_BLOCK] + \
        [("reconstruct", kw, msg) for kw, msg in [({"drop": ("d", "valid")}, "NULL argument (linear_rgb"), ({"drop": ("valid",), "height": 0}, "valid is NULL")] +
         DENOISE_BLOCK] + \
        [("denoise_nlm", kw, msg) for kw, msg in [
            ({"drop": ("d", "var_b")}, "NULL argument (half_a, half_b or d)"),
            ({"drop": ("var_b",), "width": 0}, "var_a and var_b go together"),
            ({"width": 0, "d": {"search_radius": 17}}, "width * height"),
            ({"d": {"search_radius": 17, "patch_radius": 5}}, "d->search_radius"),
            ({"d": {"patch_radius": 5, "reserved0": 1}}, "d->patch_radius"),
            ({"d": {"reserved1": 1, "k": NAN}}, "d->reserved0 and d->reserved1")]] + \
        [("denoise_select", kw, msg) for kw, msg in [
            ({"drop": ("half_a", "albedo")}, "NULL argument (half_a or half_b)"),
            ({"drop": ("alpha", "dn")}, "NULL argument (albedo, normal, depth or alpha)"),
            ({"drop": ("nl", "sel")}, "NULL argument (dn or nl)"),
            ({"drop": ("sel", "var_a")}, "sel is NULL"),
            ({"drop": ("var_a",), "width": 0}, "var_a and var_b go together"),
            ({"height": 0, "dn": {"iterations": 9}}, "width * height"),
            ({"dn": {"iterations": 9, "reserved0": 1}}, "dn->iterations"),
            ({"dn": {"reserved0": 1, "sigma_depth": NAN}}, "dn->reserved0"),
            ({"dn": {"sigma_luminance": -1.0}, "nl": {"search_radius": 17}}, "the sigmas (dn->sigma_luminance"),
            ({"nl": {"search_radius": 17, "patch_radius": 5}}, "nl->search_radius"),
            ({"nl": {"reserved0": 1, "k": -1.0}}, "nl->reserved0"),
            ({"nl": {"k": NAN}, "sel": {"error_radius": 17}}, "nl->k"),
            ({"sel": {"error_radius": 17, "blend_radius": 9}}, "sel->error_radius"),
            ({"sel": {"blend_radius": 9, "reserved0": 1}}, "sel->blend_radius"),
            ({"sel": {"reserved0": 1, "margin": 3.0}}, "sel->reserved0")]] + \
        [("denoise_regress", kw, msg) for kw, msg in [
            ({"drop": ("half_b", "g")}, "NULL argument (half_a or half_b)"),
            ({"drop": ("g", "var_a")}, "g is NULL"),
            ({"drop": ("var_b",), "width": 0}, "var_a and var_b go together"),
            ({"width": 0, "g": {"search_radius": 17}}, "width * height"),
            ({"g": {"search_radius": 17, "patch_radius": 5}}, "g->search_radius"),
            ({"g": {"patch_radius": 5, "k": -1.0}}, "g->patch_radius"),
            ({"g": {"k": NAN, "features": 8}}, "g->k"),
            ({"g": {"features": 8, "ridge": -1.0}}, "g->features"),
            ({"g": {"ridge": NAN, "reserved0": 1}}, "g->ridge"),
            ({"g": {"reserved1": 1, "features": 1}, "drop": ("alpha",)}, "g->reserved0 and g->reserved1"),
            ({"g": {"features": 1}, "drop": ("alpha", "albedo")}, "alpha is NULL"),
            ({"g": {"features": 3}, "drop": ("albedo", "normal")}, "albedo is NULL"),
            ({"g": {"features": 6}, "drop": ("normal", "depth")}, "normal is NULL"),
            ({"g": {"features": 4, "demodulate": 1}, "drop": ("depth", "albedo")}, "depth is NULL")]] + \
        [("temporal_accumulate", kw, msg) for kw, msg in T_AND_BEFORE + [
            ({"drop": ("linear_rgb", "depth")}, "linear_rgb is NULL"),
            ({"drop": ("prev_cam", "variance_rgb")}, "prev_cam is NULL"),
            ({"drop": ("variance_rgb",), "t": {"max_history": 65536}}, "variance_rgb and prev_variance_rgb go together")]] + \
        [("temporal_variance", kw, msg) for kw, msg in T_AND_BEFORE + V_BLOCK + [({"drop": ("v",), "width": 0}, "width * height")]] + \
        [("temporal_clamp", kw, msg) for kw, msg in T_AND_BEFORE + V_BLOCK + [
            ({"v": {"sigma_normal": -1.0}, "drop": ("k",)}, "the sigmas (v->sigma_normal"),
            ({"drop": ("v", "k")}, "v is NULL"),
            ({"k": {"radius": 5, "reserved0": 1}}, "k->radius")]] + \
        [("temporal_probe", kw, msg) for kw, msg in T_AND_BEFORE + [
            ({"t": {"normal_min": -2.0}, "drop": ("a",)}, "t->normal_min"),
            ({"a": {"boost": 3, "reserved0": 1}}, "a->boost"),
            ({"a": {"reserved0": 1, "fill": 0.5}}, "a->reserved0")]] + \
        [("svgf_create", kw, msg) for kw, msg in [
            ({"drop": ("q", "out")}, "q is NULL"),
            ({"drop": ("out",), "width": 0}, "out is NULL"),
            ({"width": 0, "q": {"t.max_history": 65536}}, "width * height"),
            ({"q": {"t.max_history": 65536, "t.reserved0": 1}}, "q->t.max_history"),
            ({"q": {"t.normal_min": NAN, "v.min_temporal": 1}}, "q->t.normal_min"),
            ({"q": {"v.radius": 5, "v.reserved0": 1}}, "q->v.radius"),
            ({"q": {"v.sigma_depth": -1.0, "d.iterations": 9}}, "the sigmas (q->v.sigma_normal"),
            ({"q": {"d.iterations": 9, "d.reserved0": 1}}, "q->d.iterations"),
            ({"q": {"d.sigma_normal": NAN, "feedback_iterations": 1}}, "the sigmas (q->d.sigma_luminance"),
            ({"q": {"feedback_iterations": 1, "demodulate": 2}}, "q->feedback_iterations"),
            ({"q": {"demodulate": 2, "reserved0": 1}}, "q->demodulate")]] + \
        [("svgf_push", kw, msg) for kw, msg in [  # (the handle is NULL in every call: it is checked last)
            ({"drop": ("cam", "linear_rgb")}, "cam is NULL"),
            ({"drop": ("linear_rgb", "albedo")}, "linear_rgb is NULL"),
            ({"drop": ("depth",)}, "NULL argument (albedo, normal, depth or alpha)"),
            ({}, "q is NULL")]] + \
        [("svgf_frame", kw, msg) for kw, msg in [
            ({"drop": ("cam", "p")}, "cam is NULL"),
            ({"drop": ("p",)}, "p is NULL"),
            ({"p": {"reserved0": 1, "tile_world": 2}}, "reserved0 must be 0"),
            ({"p": {"tile_world": 2}}, "tile_world"),
            ({}, "q is NULL")]]


@pytest.mark.parametrize("name,kw,msg", CASES, ids=["%s-%d" % (c[0], i) for i, c in enumerate(CASES)])
def test_the_earlier_of_two_faults_is_reported(name, kw, msg):
    assert call(name, **kw) == INVALID, (name, kw)
    err = library.product().last_error().decode()
    assert err.startswith(name + ": ") and msg in err, (kw, err)


def test_a_refusal_keeps_its_code_in_front_of_the_handle():
    """rttnw_svgf_frame's one refusal with another code stands where it stood: behind reserved0 and tile_world, in front of the NULL handle."""
    assert call("svgf_frame", p={"collect_counters": 1}) == UNSUPPORTED
    assert library.product().last_error().decode().startswith("svgf_frame: collect_counters")


def test_every_entry_point_is_covered():
    assert {c[0] for c in CASES} == {"denoise", "reconstruct", "denoise_nlm", "denoise_select", "denoise_regress", "temporal_accumulate",
                                    "temporal_variance", "temporal_clamp", "temporal_probe", "svgf_create", "svgf_push", "svgf_frame"}
