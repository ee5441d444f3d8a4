"""Run-ahead in the walk trips of the lane-owns-path kernel (trace_kernel_plain RUN_AHEAD, rt_core.hpp trav_trip_ahead) on the MI355X: the timed `plain`
instantiation with RTTNW_RUN_AHEAD on against the same with it off — two instantiations of one build, held to the project's bounds for such a pair
(tests/test_gpu_parity.py::test_kernel_forms_agree): RTTNW_F64_STRICT bit-identical, f64 within 1e-9 with RGBA8 equal, f32 at most 0.2 % of the
pixels differing.  The scenes are tests/run_ahead_cases.py's (the host build drives the same walks to completion in tests/test_run_ahead_cpu.py);
final_scene at the forms test's 72x56 spp 6, spp_chunk 2.  rttnw_stats.reserved bit 7 says run-ahead ran exactly when the plan chose it."""
import numpy as np
import pytest

import run_ahead_cases
from rttnw_amd import abi, render
from rttnw_amd import scene as S

pytestmark = pytest.mark.gpu
PRECISIONS = [abi.F64_STRICT, abi.F64, abi.F32]
RUN_AHEAD = 128   # launch_plan.hpp FORM_RUN_AHEAD


@pytest.fixture
def hostsim():
    """The host build with hostsim_plan_run_ahead: tests/hostsim's code in a library of its own (tests/run_ahead_host)."""
    return run_ahead_cases.host_binding()


def _plan(hostsim, sc_host, precision, override, listed=0):
    v = hostsim.lib.hostsim_plan_run_ahead(sc_host.handle, 4 if precision == abi.F32 else 8, 0, listed, 1, override)   # (forced: plain)
    assert v >= 0
    return v & 1


def _same(precision, a, b, what):
    if precision == abi.F64_STRICT:
        assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1]), what
    elif precision == abi.F64:
        d = np.abs(a[0] - b[0])
        assert np.nanmax(d) <= 1e-9 and np.array_equal(np.isnan(a[0]), np.isnan(b[0])) and np.array_equal(a[1], b[1]), (what, np.nanmax(d))
    else:
        assert (np.nan_to_num(np.abs(a[0] - b[0])).max(axis=2) > 0).mean() <= 2e-3, what


@pytest.mark.parametrize("name", run_ahead_cases.NAMES)
def test_run_ahead_on_against_off(gpu, hostsim, scenes_lib, earth, name, monkeypatch):
    monkeypatch.setenv("RTTNW_KERNEL", "plain")
    sc, cam, make = run_ahead_cases.case(gpu, scenes_lib, earth, name)
    sc_host = run_ahead_cases.case(hostsim, scenes_lib, earth, name)[0]
    chose = 0
    for precision in PRECISIONS:
        if name == "final_scene":
            cam, p = S.params_for(sc.setup, 72, 56, 6, spp_chunk=2, precision=precision, seed=11)
        else:
            p = make(precision)
        out = {}
        for override in ("0", "1", None):
            if override is None:
                monkeypatch.delenv("RTTNW_RUN_AHEAD", raising=False)
            else:
                monkeypatch.setenv("RTTNW_RUN_AHEAD", override)
            lin, rgba, st = render.render_host(sc, cam, p)
            planned = _plan(hostsim, sc_host, precision, -1 if override is None else int(override))
            assert ((st.reserved & RUN_AHEAD) != 0) == (planned == 1), (name, precision, override, st.reserved)
            assert (st.reserved & 1) == 0 and st.samples == p.width * p.height * p.spp
            out[override] = (lin, rgba)
            chose += planned if override == "1" else 0
        for override in ("1", None):
            _same(precision, out[override], out["0"], (name, precision, override))
    assert chose == len(PRECISIONS), name   # none of these walks changes frames: the override turned run-ahead on for every one of them


def test_a_region_window_is_the_crop_of_the_frame_with_run_ahead(gpu, scenes_lib, earth, monkeypatch):
    """The LIST twin: one rttnw_render_region window of final_scene — tests/test_gpu_region.py's frame and its smallest window, the one pixel of the
    partial corner tile — equals the crop of the frame bit for bit with run-ahead on, in every precision."""
    monkeypatch.delenv("RTTNW_KERNEL", raising=False)
    monkeypatch.setenv("RTTNW_RUN_AHEAD", "1")
    sc, setup = S.build(gpu, scenes_lib, "final_scene", earth)
    win = (39, 27, 40, 28)
    for precision in PRECISIONS:
        cam, p = S.params_for(setup, 40, 28, 32, precision=precision, spp_chunk=2)
        lin, rgba, st = render.render_host(sc, cam, p)
        l, r, rst = render.render_region(sc, cam, p, *win)
        assert (st.reserved & RUN_AHEAD) != 0 and rst.reserved == st.reserved, (st.reserved, rst.reserved)
        assert np.array_equal(l, lin[27:28, 39:40]) and np.array_equal(r, rgba[27:28, 39:40]), precision
        assert rst.samples == p.spp
