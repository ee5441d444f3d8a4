"""rttnw_render_features and rttnw_denoise without a GPU: the exports exist and are declared alike in the header, the ctypes binding
and the Rust binding, and every argument refusal comes before the device is touched."""
import ctypes as C
import re

import numpy as np
import pytest

from abi_cases import FFI, HEADER, camera, exported, params
from rttnw_amd import abi, library
from rttnw_amd import scene as S


def test_exports_and_declarations():
    for name in ("rttnw_render_features", "rttnw_denoise"):
        exported(name[len("rttnw_"):])
        assert re.search(r"\bint %s\(" % name, HEADER) and re.search(r"pub fn %s\(" % name, FFI)
    body = re.search(r"struct rttnw_denoise_params \{(.*?)\};", HEADER, flags=re.S).group(1)
    names = [n.strip() for _, group in re.findall(r"(uint32_t|double)\s+([\w, ]+);", body) for n in group.split(",")]
    assert names == ["iterations", "reserved0", "sigma_luminance", "sigma_normal", "sigma_depth"]
    assert "typedef struct rttnw_denoise_params rttnw_denoise_params;" in HEADER
    rs_body = re.search(r"pub struct rttnw_denoise_params \{(.*?)\n\}", FFI, flags=re.S).group(1)
    assert re.findall(r"pub (\w+): (\w+),", rs_body) == [("iterations", "u32"), ("reserved0", "u32"), ("sigma_luminance", "f64"),
                                                         ("sigma_normal", "f64"), ("sigma_depth", "f64")]
    assert [n for n, _ in abi.Denoise._fields_] == names
    assert C.sizeof(abi.Denoise) == 32 and abi.Denoise.sigma_luminance.offset == 8 and abi.Denoise.sigma_depth.offset == 24


# ---------------------------------------------------------------------------------------------- rttnw_render_features

def _features(b, sc, p):
    cam = camera()
    return b.render_features(sc.handle, C.byref(cam), C.byref(p) if p is not None else None, None, None, None, None, None)


@pytest.mark.parametrize("what,kw,code,msg", [
    ("spp 0", {"spp": 0}, -1, "spp is 0"),
    ("reserved0", {"reserved0": 1}, -1, "reserved0"),
    ("tile_world", {"tile_world": 2}, -1, "tile_world"),
    ("counters", {"collect_counters": 1}, -3, "collect_counters"),
])
def test_feature_refusals_come_before_the_device(what, kw, code, msg):
    b = library.product()
    sc = S.Scene(b)                                   # never committed: a device would be needed for that
    kw.setdefault("spp", 4)
    p = params(**kw)
    assert _features(b, sc, p) == code, what
    assert msg in b.last_error().decode(), (what, b.last_error())


def test_valid_feature_arguments_reach_the_scene_checks():
    b = library.product()
    sc = S.Scene(b)
    assert _features(b, sc, None) == -1 and "NULL" in b.last_error().decode()
    assert _features(b, sc, params(spp=4)) == -2   # RTTNW_ERR_STATE: the scene is not committed
    assert "not committed" in b.last_error().decode()
    cam = camera()
    p = params(spp=4)
    assert b.render_features(None, C.byref(cam), C.byref(p), None, None, None, None, None) == -1


# ---------------------------------------------------------------------------------------------- rttnw_denoise

def _denoise(b, w=8, h=8, drop=None, **kw):
    a = {k: np.full((h, w, 3) if k in ("linear", "albedo", "normal") else (h, w), 0.5) for k in ("linear", "albedo", "normal", "depth", "alpha")}
    d = abi.Denoise(iterations=kw.pop("iterations", 2), reserved0=kw.pop("reserved0", 0), sigma_luminance=kw.pop("sigma_luminance", 0.0),
                    sigma_normal=kw.pop("sigma_normal", 0.0), sigma_depth=kw.pop("sigma_depth", 0.0))
    ptr = {k: (None if k == drop else v.ctypes.data) for k, v in a.items()}
    out = np.zeros((h, w, 3))
    return b.denoise(w, h, ptr["linear"], None, ptr["albedo"], ptr["normal"], ptr["depth"], ptr["alpha"],
                     None if drop == "d" else C.byref(d), out.ctypes.data, None, None, None)


@pytest.mark.parametrize("what,kw,msg", [
    ("no image", {"drop": "linear"}, "NULL"), ("no albedo", {"drop": "albedo"}, "NULL"), ("no normal", {"drop": "normal"}, "NULL"),
    ("no depth", {"drop": "depth"}, "NULL"), ("no alpha", {"drop": "alpha"}, "NULL"), ("no parameters", {"drop": "d"}, "NULL"),
    ("empty", {"w": 0}, "empty image"), ("empty", {"h": 0}, "empty image"),
    ("iterations", {"iterations": 9}, "iterations"), ("reserved0", {"reserved0": 7}, "reserved0"),
    ("negative sigma", {"sigma_depth": -1.0}, "sigmas"), ("negative sigma", {"sigma_normal": -0.5}, "sigmas"),
    ("NaN sigma", {"sigma_luminance": float("nan")}, "sigmas"),
])
def test_denoise_refusals_come_before_the_device(what, kw, msg):
    b = library.product()
    assert _denoise(b, **kw) == -1, what
    assert msg in b.last_error().decode(), (what, b.last_error())


@pytest.mark.skipif(library.product().device_count() > 0, reason="a GPU is present")
def test_denoise_has_no_cpu_fallback():
    b = library.product()
    assert _denoise(b) == -4                                   # RTTNW_ERR_HIP
    assert "no CPU fallback" in b.last_error().decode()
