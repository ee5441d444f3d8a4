"""The host build's set-up path — scene records, camera and render constants of one precision (rttnw_amd/csrc/scene_narrow.hpp, the
set-up helper of tests/hostsim/hostsim.cpp) and the probe loop (rt_core.hpp probe_path) — pinned to the bytes it produced before these
were shared with the device build: cornell_box at 8 x 8, spp 4, both precisions.  tests/golden/host_setup_pins.npz holds capture()'s
arrays as the commit before that change made them (cornell_box needs no libm function, so the bytes do not depend on the C library)."""
import ctypes as C
import os

import numpy as np

import util
from rttnw_amd import abi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host_setup_pins.npz")
MAX_OUT = 16


def capture(hostsim, scenes_lib):
    """{name: array}: per precision the 8 x 8 image, and of sample 0 of every pixel the probe's whole output buffer and record count."""
    fn = hostsim.lib.hostsim_probe_path
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(abi.CameraDesc), C.POINTER(abi.Params), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32]
    sc, setup = util.build(hostsim, scenes_lib, "cornell_box")
    out = {}
    for tag, precision in (("f32", abi.F32), ("f64", abi.F64)):
        cam, p = util.params_for(setup, 8, 8, 4, seed=11, precision=precision)
        out["image_" + tag], _ = util.hostsim_render(hostsim, sc, cam, p, n_threads=2)
        probes, counts = np.zeros((64, MAX_OUT * util.PROBE_STRIDE + 4)), np.zeros(64, dtype=np.int32)
        for i in range(64):
            counts[i] = fn(sc.handle, C.byref(cam), C.byref(p), i % 8, i // 8, 0, probes[i].ctypes.data, MAX_OUT)
        out["probes_" + tag], out["counts_" + tag] = probes, counts
    return out


def test_host_setup_and_probe_give_the_pinned_bytes(hostsim, scenes_lib):
    got, want = capture(hostsim, scenes_lib), np.load(GOLDEN)
    assert sorted(got) == sorted(want.files)
    for name in want.files:
        assert got[name].dtype == want[name].dtype and got[name].tobytes() == want[name].tobytes(), name
    assert got["counts_f64"].max() > 1 and np.abs(got["image_f32"] - got["image_f64"]).max() > 0.0   # paths that bounce; two precisions
