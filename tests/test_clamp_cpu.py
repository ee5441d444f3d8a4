"""rttnw_temporal_clamp without a GPU: the host build of the arithmetic the device kernel runs (rttnw_amd/csrc/clamp.hpp, built by
tests/clamp_host) against a numpy restatement of the contract in include/rttnw_hip.h — bit for bit, every output, along chains of three calls —
and the properties the contract promises: a ghost goes in one frame, honest noise stays, the window stops at edges, misses pass through and enter no
window; with gamma = +inf the call is rttnw_temporal_variance."""
import numpy as np
import pytest

import clamp_ref
import variance_ref
from temporal_cases import same
from clamp_cases import (CASE_IDS, CASES, assert_same_outputs, case_parameters, chain, check_a_ghost_goes, check_chain, check_miss_pixels,
                         check_noise_stays, check_the_window_respects_edges)


@pytest.fixture(scope="module")
def host():
    return clamp_ref.host()


def test_the_cases_are_the_stated_matrix():
    assert len(CASES) == 36 and len(set(CASE_IDS)) == 36
    assert sum(1 for c in CASES if c[7]) == 9                             # a quarter carry NaN and inf
    for size in {c[0] for c in CASES}:
        assert {(c[1], c[2]) for c in CASES if c[0] == size} == {(r, g) for r in (1, 3, 4) for g in (0.25, 1.0, float("inf"))}


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_host_build_equals_the_numpy_restatement_bit_for_bit(host, case):
    """... and the restatement meets the cases' condition: something is clipped and something with a history is not (finite gamma, 37x29 and up);
    nothing is clipped and the shared outputs are variance_ref's (gamma = +inf)."""
    clipped, unclipped = check_chain(host, case)
    print("clipped channels %d, unclipped pixels with a history %d" % (clipped, unclipped))


def test_gamma_inf_equals_the_host_build_of_temporal_variance(host):
    """The two host builds against each other: with gamma = +inf the sibling functions compute what variance.hpp computes."""
    plain = variance_ref.host()
    for case in (c for c in CASES if np.isinf(c[2]) and c[0] == (70, 41)):
        history, frames = chain(case)
        kw = case_parameters(case)
        vkw = {k: kw[k] for k in ("max_history", "min_temporal", "normal_min", "radius")}
        for lin, f, cam in frames:
            nxt = host(lin, f, cam, history=history, **kw)
            assert_same_outputs(nxt, plain(lin, f, cam, history=history, **vkw), names=clamp_ref.SHARED)
            assert not nxt["clipped"].any()
            history = nxt


def test_zero_parameters_are_the_stated_defaults(host):
    history, frames = chain(CASES[-2])
    lin, f, cam = frames[0]
    default = host(lin, f, cam, history=history)
    assert_same_outputs(default, host(lin, f, cam, history=history, gamma=1.0, clamp_radius=3, clamp_sigma_normal=64.0, clamp_sigma_depth=0.1,
                                      max_history=32, depth_tolerance=0.05, normal_min=0.9, min_temporal=4, radius=3, sigma_normal=64.0, sigma_depth=0.1))
    for other in ({"gamma": 2.0}, {"clamp_radius": 1}, {"clamp_sigma_normal": 2.0}, {"clamp_sigma_depth": 1.0}):
        assert not np.array_equal(default["linear"], host(lin, f, cam, history=history, **other)["linear"]), other


def test_no_history_is_this_frame_and_clips_nothing(host):
    history, frames = chain(CASES[-2])
    lin, f, cam = frames[0]
    for run in (host, clamp_ref.clamp):
        first = run(lin, f, cam)
        assert same(first["linear"], lin) and same(first["moment2"], lin * lin)
        assert np.all(first["length"] == 1.0) and np.isnan(first["prev_xy"]).all() and not first["clipped"].any()
        assert np.all((first["sd"] >= 0.0) | np.isnan(first["sd"]))                 # (a NaN colour makes the deviations of its window NaN)


def test_a_ghost_goes(host):
    check_a_ghost_goes(host, variance_ref.host())
    check_a_ghost_goes(clamp_ref.clamp, variance_ref.estimate)


def test_noise_stays(host):
    print("share of clipped channels per frame, variance * 8 over sigma^2 (left, right):", check_noise_stays(host))


def test_the_window_respects_edges(host):
    check_the_window_respects_edges(host)


def test_miss_pixels_pass_through_and_enter_no_window(host):
    check_miss_pixels(host)
