"""rttnw_render_adaptive without a GPU: the declarations agree across the header, the ctypes binding and the Rust binding, every
argument refusal comes before the device is touched, and the noise estimate / stopping rule the kernels include
(rttnw_amd/csrc/adaptive.hpp, built on the host by tests/adaptive_host) matches a numpy statement of it."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from abi_cases import FFI, HEADER, ROOT, adaptive, camera, exported, params
from rttnw_amd import abi, library
from rttnw_amd import scene as S


class AdaptivePixel(C.Structure):
    """rt::AdaptivePixel (adaptive.hpp)."""
    _fields_ = [("mu", C.c_double * 3), ("m2", C.c_double * 3), ("n", C.c_uint32), ("k", C.c_uint32)]


@pytest.fixture(scope="module")
def host():
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "adaptive_host"), "-s"], check=True)
    lib = C.CDLL(os.path.join(ROOT, "tests", "adaptive_host", "libadaptive_host.so"))
    lib.ah_fold.argtypes = [C.POINTER(AdaptivePixel), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    lib.ah_fold.restype = None
    lib.ah_stderr.argtypes = [C.POINTER(AdaptivePixel), C.c_int]
    lib.ah_stderr.restype = C.c_double
    lib.ah_active.argtypes = [C.POINTER(AdaptivePixel), C.c_void_p, C.c_double, C.c_double, C.c_uint32]
    lib.ah_active.restype = C.c_int
    return lib


# ---------------------------------------------------------------------------------------------- declarations

def test_struct_and_entry_point_are_declared_alike_everywhere():
    body = re.search(r"struct rttnw_adaptive \{(.*?)\};", HEADER, flags=re.S).group(1)
    c_fields = re.findall(r"(uint32_t|double)\s+(\w+);", body)
    assert [n for _, n in c_fields] == ["pass_spp", "reserved0", "rel_error", "abs_error"]
    assert "typedef struct rttnw_adaptive rttnw_adaptive;" in HEADER
    rs_body = re.search(r"pub struct rttnw_adaptive \{(.*?)\n\}", FFI, flags=re.S).group(1)
    rs_fields = re.findall(r"pub (\w+): (\w+),", rs_body)
    to_rs = {"uint32_t": "u32", "double": "f64"}
    assert rs_fields == [(n, to_rs[t]) for t, n in c_fields]
    assert [(n, t) for n, t in abi.Adaptive._fields_] == [("pass_spp", C.c_uint32), ("reserved0", C.c_uint32),
                                                         ("rel_error", C.c_double), ("abs_error", C.c_double)]
    assert C.sizeof(abi.Adaptive) == 24 and abi.Adaptive.rel_error.offset == 8 and abi.Adaptive.abs_error.offset == 16
    sig = re.search(r"int rttnw_render_adaptive\((.*?)\);", HEADER, flags=re.S).group(1)
    assert len(sig.split(",")) == 9
    rs_sig = re.search(r"pub fn rttnw_render_adaptive\((.*?)\) -> c_int;", FFI, flags=re.S).group(1)
    assert "a: *const rttnw_adaptive" in rs_sig and "out_spp: *mut u32" in rs_sig and "out_stderr_rgb: *mut f64" in rs_sig
    exported("render_adaptive")


# ---------------------------------------------------------------------------------------------- refusals

def _call(b, sc, p, a):
    cam = camera()
    return b.render_adaptive(sc.handle, C.byref(cam), C.byref(p), C.byref(a) if a is not None else None,
                             None, None, None, None, None)


@pytest.mark.parametrize("what,kw,adapt,code,msg", [
    ("pass_spp 0", {}, dict(pass_spp=0), abi.RTTNW_OK - 1, "pass_spp is 0"),
    ("cap not a multiple", {"spp": 96}, dict(pass_spp=64), -1, "multiple of pass_spp"),
    ("cap 0", {"spp": 0}, dict(pass_spp=64), -1, "multiple of pass_spp"),
    ("negative rel", {}, dict(rel_error=-0.1), -1, "rel_error and abs_error"),
    ("NaN abs", {}, dict(abs_error=float("nan")), -1, "rel_error and abs_error"),
    ("reserved0", {}, dict(reserved0=1), -1, "reserved0"),
    ("tile_world", {"tile_world": 2}, {}, -1, "tile_world"),
    ("counters", {"collect_counters": 1}, {}, -3, "collect_counters"),
])
def test_refusals_come_before_the_device(what, kw, adapt, code, msg):
    b = library.product()
    sc = S.Scene(b)                                   # never committed: a device would be needed for that
    p, a = params(**kw), adaptive(**adapt)
    assert _call(b, sc, p, a) == code, what
    assert msg in b.last_error().decode(), (what, b.last_error())


def test_valid_arguments_reach_the_scene_checks():
    b = library.product()
    sc = S.Scene(b)
    p = params()
    assert _call(b, sc, p, None) == abi.RTTNW_OK - 1          # NULL rule
    a = adaptive()
    assert _call(b, sc, p, a) == -2                           # RTTNW_ERR_STATE: the scene is not committed
    assert "not committed" in b.last_error().decode()


# ---------------------------------------------------------------------------------------------- the estimator

def _sequence(rng, k):
    n = rng.choice([1, 2, 4, 5, 16], size=k).astype(np.uint32)
    # heavy-tailed radiance-like chunk means: mostly small, some large, some zero
    m = rng.exponential(0.3, size=(k, 3)) * (rng.random((k, 1)) < 0.9) + (rng.random((k, 3)) < 0.05) * rng.exponential(20.0, size=(k, 3))
    return np.ascontiguousarray(m, dtype=np.float64), np.ascontiguousarray(n)


def _fold(host, m, n, splits):
    st = AdaptivePixel()
    for c0, c1 in zip(splits[:-1], splits[1:]):
        host.ah_fold(C.byref(st), m.ctypes.data, n.ctypes.data, c0, c1)
    return st


def test_m2_and_stderr_match_numpy(host):
    rng = np.random.default_rng(7)
    for trial in range(200):
        k = int(rng.integers(2, 120))
        m, n = _sequence(rng, k)
        st = _fold(host, m, n, [0, k])
        N = float(n.sum())
        mu = (m * n[:, None]).sum(axis=0) / N
        m2 = (n[:, None] * (m - mu) ** 2).sum(axis=0)
        se = np.sqrt(m2 / ((k - 1) * N))
        assert st.n == int(n.sum()) and st.k == k
        for ch in range(3):
            assert st.mu[ch] == pytest.approx(mu[ch], rel=1e-12, abs=1e-300)
            assert st.m2[ch] == pytest.approx(m2[ch], rel=1e-12, abs=1e-12 * max(m2[ch], 1e-300) + 1e-280)
            assert host.ah_stderr(C.byref(st), ch) == pytest.approx(se[ch], rel=1e-12, abs=1e-300)


def test_one_sample_chunks_give_the_textbook_standard_error(host):
    rng = np.random.default_rng(3)
    x = np.ascontiguousarray(rng.exponential(1.0, size=(50, 3)))
    n = np.ones(50, dtype=np.uint32)
    st = _fold(host, x, n, [0, 50])
    want = x.std(axis=0, ddof=1) / math.sqrt(50)
    for ch in range(3):
        assert host.ah_stderr(C.byref(st), ch) == pytest.approx(want[ch], rel=1e-12)


def test_state_carried_across_any_split_is_bit_identical(host):
    rng = np.random.default_rng(11)
    for trial in range(100):
        k = int(rng.integers(1, 80))
        m, n = _sequence(rng, k)
        whole = bytes(_fold(host, m, n, [0, k]))
        cuts = sorted(set(rng.integers(0, k + 1, size=int(rng.integers(0, 6))).tolist()) | {0, k})
        assert bytes(_fold(host, m, n, cuts)) == whole, cuts


def test_fewer_than_two_chunks_is_infinite_and_never_converged(host):
    m = np.ascontiguousarray([[0.5, 0.5, 0.5]])
    n = np.ascontiguousarray([64], dtype=np.uint32)
    st = _fold(host, m, n, [0, 1])
    assert all(math.isinf(host.ah_stderr(C.byref(st), ch)) for ch in range(3))
    v = np.ascontiguousarray([0.5, 0.5, 0.5])
    assert host.ah_active(C.byref(st), v.ctypes.data, 1e9, 1e9, 128) == 1
    assert host.ah_active(C.byref(st), v.ctypes.data, 1e9, 1e9, 64) == 0       # ... until the cap
    st0 = AdaptivePixel()
    assert math.isinf(host.ah_stderr(C.byref(st0), 0))


def test_stopping_rule_per_channel(host):
    rng = np.random.default_rng(5)
    m, n = _sequence(rng, 32)
    st = _fold(host, m, n, [0, 32])
    se = np.array([host.ah_stderr(C.byref(st), ch) for ch in range(3)])
    v = np.ascontiguousarray(np.array(st.mu[:]))
    rel = float(np.max(se / v)) * 1.0001
    assert host.ah_active(C.byref(st), v.ctypes.data, rel, 0.0, 10 ** 6) == 0
    assert host.ah_active(C.byref(st), v.ctypes.data, float(np.min(se / v)) * 0.999, 0.0, 10 ** 6) == 1   # one channel misses it
    assert host.ah_active(C.byref(st), v.ctypes.data, 0.0, float(se.max()) * 1.0001, 10 ** 6) == 0
    assert host.ah_active(C.byref(st), v.ctypes.data, 0.0, float(se.max()) * 0.999, 10 ** 6) == 1
