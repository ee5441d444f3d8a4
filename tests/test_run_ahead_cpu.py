"""Run-ahead in the walk trips of the lane-owns-path kernel (rt_core.hpp trav_trip_ahead), on the host build: tests/run_ahead_host's
hostsim_render_run_ahead drives every walk of a render through the kernel's own trips — the same stash points, the same leaf step, the same finish
rule — to completion, and holds each walk against the canonical walk of the same ray.  The host build contracts nothing, so the image must equal
the canonical render's bit for bit; the walks' bookkeeping: the canonical record tests come in the canonical order (a subsequence of the run-ahead
walk's tests: a stale `closest` may open a leaf the canonical walk culls, whose test then fails), the node steps are at least the canonical
walk's, no lane ends a trip or a walk with a record still put aside."""
import ctypes as C

import numpy as np
import pytest

import run_ahead_cases
import util
from rttnw_amd import abi

TOTALS = ("walks", "nodes_canonical", "nodes_ahead", "tests_canonical", "tests_ahead", "put_aside", "order_broken", "result_differs",
          "register_full_at_end", "done_while_put_aside", "fewer_nodes", "trips", "twin_differs")


def run_ahead_render(hostsim, sc, cam, p, node_steps):
    lib = hostsim.lib
    lin = np.zeros((p.height, p.width, 3))
    tot = np.zeros(len(TOTALS), dtype=np.uint64)
    assert lib.hostsim_render_run_ahead(sc.handle, C.byref(cam), C.byref(p), node_steps, lin.ctypes.data, tot.ctypes.data, 0) == 0
    return lin, {k: int(v) for k, v in zip(TOTALS, tot)}


_CASES = {}


@pytest.fixture
def hostsim():
    """The host build with the run-ahead drivers: tests/hostsim's code in a library of its own (tests/run_ahead_host)."""
    return run_ahead_cases.host_binding()


@pytest.fixture
def cases(hostsim, scenes_lib, earth):
    def get(name):
        if name not in _CASES:   # the scene and its canonical render: made once, never written to
            sc, cam, make = run_ahead_cases.case(hostsim, scenes_lib, earth, name)
            ref = {}
            for precision in (abi.F64, abi.F32):
                ref[precision], _ = util.hostsim_render(hostsim, sc, cam, make(precision))
                ref[precision].setflags(write=False)
            _CASES[name] = (sc, cam, make, ref)
        return _CASES[name]
    return get


@pytest.mark.parametrize("node_steps", [2, 3])
@pytest.mark.parametrize("name", run_ahead_cases.NAMES)
def test_run_ahead_walks_render_the_canonical_image(hostsim, cases, name, node_steps):
    sc, cam, make, ref = cases(name)
    for precision in (abi.F64, abi.F32):
        lin, t = run_ahead_render(hostsim, sc, cam, make(precision), node_steps)
        print(name, node_steps, "f64" if precision == abi.F64 else "f32", t)
        assert np.array_equal(lin, ref[precision], equal_nan=True), (name, precision, np.nanmax(np.abs(lin - ref[precision])))
        assert t["walks"] > 0 and t["result_differs"] == 0 and t["order_broken"] == 0, t
        assert t["register_full_at_end"] == 0 and t["twin_differs"] == 0, t   # (the image's walks go through trav_trip_ahead itself; the log is its twin's)
        assert t["fewer_nodes"] == 0 and t["nodes_ahead"] >= t["nodes_canonical"] and t["tests_ahead"] >= t["tests_canonical"], t
        # the stale `closest` costs a few per cent of visits, not a different walk
        assert t["nodes_ahead"] <= 1.25 * t["nodes_canonical"] + t["walks"], t
        # (the one sphere is reached by a node step and tested by that trip's leaf step: with the stash point at the trip's start alone nothing is put
        # aside there; of two spheres the second comes off the stack at a leaf step's end and is put aside at the next trip's start)
        if name != "one":
            assert t["put_aside"] > 0, t
        if name == "two":
            assert t["done_while_put_aside"] > 0, t   # a pop found the stack empty while the lane's record was put aside


def test_the_cases_cover_what_they_are_there_for(hostsim, cases):
    dims = (C.c_uint32 * 8)()
    sc = cases("final_scene")[0]
    assert hostsim.lib.hostsim_scene_dims(sc.handle, dims) == 0
    assert dims[7] > 16, dims[7]   # stack entries beyond the 16 a lane keeps in LDS: the spill strip is in play
    hostsim.lib.hostsim_max_stack()
    cam, make = cases("final_scene")[1:3]
    run_ahead_render(hostsim, sc, cam, make(abi.F64), 2)
    deepest_ahead = hostsim.lib.hostsim_max_stack()
    util.hostsim_render(hostsim, sc, cam, make(abi.F64))
    deepest = hostsim.lib.hostsim_max_stack()
    assert deepest_ahead <= dims[7] and deepest <= dims[7], (deepest_ahead, deepest, dims[7])
    # the tie scene: coincident pairs in both list orders show both colours of each pair (the LATER record of a pair wins its tie)
    ref = cases("ties")[3][abi.F64]
    assert np.isfinite(ref).all() and len(np.unique(ref.reshape(-1, 3), axis=0)) > 8


@pytest.mark.parametrize("name", ["final_scene", "cornell_box"])
def test_the_plan_names_run_ahead_for_walks_that_never_change_frames(hostsim, scenes_lib, earth, name):
    """launch_plan.hpp plan_launch: bits 0-5 of the plan are what they were (the existing plan tests hold them); the host build reports the plan's
    run-ahead choice through hostsim_plan_run_ahead: by itself for a scene without instance leaves (final_scene), never for a counting render, on or off
    by the override wherever the walk never changes frames; with run-ahead a trip has three node steps."""
    sc, _ = util.build(hostsim, scenes_lib, name, earth)
    lib = hostsim.lib

    def plan(real_bytes, count=0, listed=0, forced=0, override=-1):
        v = lib.hostsim_plan_run_ahead(sc.handle, real_bytes, count, listed, forced, override)
        assert v >= 0
        return v & 1, v >> 1   # (run-ahead, node steps per trip)
    own_steps = 3 if name == "cornell_box" else 2   # (without run-ahead; with it a trip has three node steps: launch_plan.hpp RUN_AHEAD_STEPS)
    for real_bytes in (4, 8):
        for listed in (0, 1):
            assert plan(real_bytes, listed=listed) == ((1, 3) if name == "final_scene" else (0, own_steps))
            assert plan(real_bytes, listed=listed, override=0) == (0, own_steps)
            assert plan(real_bytes, listed=listed, override=1) == (1, 3)
        for override in (-1, 0, 1):
            assert plan(real_bytes, count=1, override=override) == (0, 2)         # the counting instantiations keep the canonical trips
            assert plan(real_bytes, forced=2, override=override)[0] == 0          # records in global memory: the general instantiation
            assert plan(real_bytes, forced=3, override=override)[0] == 0          # the decoupled kernel
