"""rttnw_temporal_probe on the MI355X: the device kernel equals the host build of the same header (tests/probe_host) and the numpy restatement of
the contract bit for bit along the chains of tests/test_probe_cpu.py — frames that cross the kernel's 64 x 4 blocks and frames smaller than one —,
the staircase of the multiplier holds, and on the first-hit features of real scenes the device equals the host build and the call's stated
consequence holds against rttnw_temporal_accumulate on the device."""
import copy

import numpy as np
import pytest

import probe_ref
from probe_cases import CASE_IDS, CASES, assert_same_outputs, check_chain, check_staircase
from temporal_cases import same
from rttnw_amd import abi, library, render
from rttnw_amd import scene as S

pytestmark = pytest.mark.gpu
device = render.temporal_probe


@pytest.fixture(scope="module")
def host():
    return probe_ref.host()


@pytest.fixture(scope="module")
def scenes(gpu):
    lib = library.scenes()
    return {name: S.build(gpu, lib, name, S.load_earth() if name == "final_scene" else None) for name in ("cornell_box", "final_scene")}


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_device_equals_host_build_equals_the_numpy_restatement_bit_for_bit(gpu, host, case):
    """The cases of tests/test_probe_cpu.py — 70x41 crosses the 64-wide blocks and is no multiple of 4 rows, 1x1 and 3x5 are smaller than a block.
    check_chain holds the device to the restatement and the consequence; the host build is held to the device on the same links."""
    def both(f, cam, history=None, **kw):
        got = device(f, cam, history=history, **kw)
        assert_same_outputs(got, host(f, cam, history=history, **kw), ("device against host build",))
        return got
    check_chain(both, case)


def test_the_multiplier_staircase(gpu):
    check_staircase(device)


def test_kernel_time_is_reported(gpu):
    f = {"normal": np.zeros((41, 70, 3)), "depth": np.zeros((41, 70)), "alpha": np.zeros((41, 70))}
    assert device(f, S.camera_desc(lookfrom=(0, 0, 5), lookat=(0, 0, 0), vfov=40.0, aspect=70 / 41), want_ms=True)["ms"] > 0.0


@pytest.mark.parametrize("name", ["cornell_box", "final_scene"])
def test_device_equals_host_build_on_real_features(scenes, host, name):
    """96x96 features of two cameras two degrees apart, the first frame's accumulated length (all ones) as the history, then the second frame's
    (ones and twos) under a third camera: every output; the consequence against rttnw_temporal_accumulate on the device; pixels with and without a
    history both occur on hits."""
    sc, setup = scenes[name]
    cam, p = S.params_for(setup, 96, 96, 8, precision=abi.F64)
    history = None
    for k, c in enumerate(render.orbit_cameras(cam, 3, 2.0)):
        pk = copy.copy(p)
        pk.sample_begin = k * p.spp
        f = render.render_features(sc, c, pk)
        lin = np.zeros((96, 96, 3))
        for boost, fill in ((8, 8.0), (4, 3.5), (0, 0.0)):
            got = device(f, c, history=history, boost=boost, fill=fill)
            assert_same_outputs(got, host(f, c, history=history, boost=boost, fill=fill), (k, boost, fill))
        nxt = render.temporal_accumulate(lin, f, c, history=history)
        assert same(probe_ref.grown(got["length"]), nxt["length"]) and same(got["prev_xy"], nxt["prev_xy"]), k
        hit = f["alpha"] != 0.0
        if k:
            assert (hit & (got["length"] == 0.0)).any() and (hit & (got["length"] >= 1.0)).any(), k
            assert (got["multiplier"][hit] == 8).any() and (got["multiplier"][hit] < 8).any(), k
        else:
            assert np.all(got["multiplier"][hit] == 8) and np.all(got["multiplier"][~hit] == 1)
        history = nxt
