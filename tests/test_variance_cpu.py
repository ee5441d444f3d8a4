"""rttnw_temporal_variance without a GPU: the host build of the arithmetic the device kernels run (rttnw_amd/csrc/variance.hpp, built by
tests/variance_host) against a numpy restatement of the contract in include/rttnw_hip.h — bit for bit, every output, along chains of three
calls — and the properties the contract promises: stage A is rttnw_temporal_accumulate, constant input has no variance, both branches are
unbiased, the window stops at edges, misses have no variance and enter no window."""
import numpy as np
import pytest

import temporal_ref
import variance_ref
from temporal_cases import same
from variance_cases import (CASE_IDS, CASES, check_chain, check_constant_input, check_miss_pixels, check_spatial_branch_is_unbiased,
                            check_temporal_branch_is_unbiased, check_window_respects_edges, assert_same_outputs, chain, case_parameters)


@pytest.fixture(scope="module")
def host():
    return variance_ref.host()


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_host_build_equals_the_numpy_restatement_bit_for_bit(host, case):
    """... and its stage A equals the restatement of rttnw_temporal_accumulate without variances, on every link of the chain."""
    spatial, temporal = check_chain(host, variance_ref.estimate, temporal_ref.accumulate, case)
    assert spatial > 0 or case[0] == (1, 1)
    if case[0] == (70, 41) and case[2] >= case[3]:                        # (a history capped below min_temporal frames is never trusted)
        assert spatial > 100 and temporal > 100, (spatial, temporal)      # both branches were exercised


def test_stage_a_equals_the_host_build_of_temporal_accumulate(host):
    """The two host builds against each other: the sibling function computes what temporal_pixel computes."""
    plain = temporal_ref.host()
    for case in (CASES[-1], CASES[-2]):
        history, frames = chain(case)
        kw = case_parameters(case)
        for lin, f, cam in frames:
            nxt = host(lin, f, cam, history=history, **kw)
            want = plain(lin, f, cam, history=dict(history, variance=None), max_history=kw["max_history"], normal_min=kw["normal_min"])
            for name in ("linear", "rgba8", "length", "prev_xy"):
                assert same(nxt[name], want[name]), name
            history = nxt


def test_zero_parameters_are_the_stated_defaults(host):
    history, frames = chain(CASES[-1])
    lin, f, cam = frames[0]
    default = host(lin, f, cam, history=history)
    assert_same_outputs(default, host(lin, f, cam, history=history, max_history=32, depth_tolerance=0.05, normal_min=0.9, min_temporal=4, radius=3,
                                      sigma_normal=64.0, sigma_depth=0.1))
    for other in ({"min_temporal": 2}, {"radius": 1}, {"sigma_normal": 2.0}, {"sigma_depth": 1.0}):
        assert not np.array_equal(default["variance"], host(lin, f, cam, history=history, **other)["variance"]), other


def test_no_history_is_this_frame_and_its_square(host):
    history, frames = chain(CASES[-1])
    lin, f, cam = frames[0]
    for run in (host, variance_ref.estimate):
        first = run(lin, f, cam)
        assert np.array_equal(first["linear"], lin) and np.array_equal(first["moment2"], lin * lin)
        assert np.all(first["length"] == 1.0) and np.isnan(first["prev_xy"]).all()


def test_constant_input_has_no_variance(host):
    check_constant_input(host)
    check_constant_input(variance_ref.estimate)


def test_the_temporal_branch_is_unbiased(host):
    print("temporal branch, variance * 8 over sigma^2 (left, right):", check_temporal_branch_is_unbiased(host))


def test_the_spatial_branch_is_unbiased(host):
    print("spatial branch, variance over sigma^2 (left, right):", check_spatial_branch_is_unbiased(host))


def test_the_window_respects_edges(host):
    check_window_respects_edges(host)


def test_miss_pixels_have_no_variance_and_enter_no_window(host):
    check_miss_pixels(host)
