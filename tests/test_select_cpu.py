"""rttnw_denoise_select without a GPU: the host build of the arithmetic the device kernels run (rttnw_amd/csrc/select.hpp over the host builds of
the two filters, built by tests/select_host) against a numpy restatement of the contract in include/rttnw_hip.h — bit for bit, every output —
and the properties the contract promises: the composition of the two existing filters at the extreme margins, a NaN of the filter that was not
chosen kept out, the exchange of the two halves, locality, and a selection that sides with the better filter where the truth is known."""
import numpy as np
import pytest

import denoise_ref
import nlm_ref
import select_ref
from select_cases import (FILTER_IDS, FILTER_SETS, MARGINS, RADII, assert_same_outputs, check_composition, check_exchange, check_locality,
                          check_unchosen_nan_stays_out, filter_set_inputs, inputs)


@pytest.fixture(scope="module")
def host():
    return select_ref.host()


@pytest.mark.parametrize("case", FILTER_SETS, ids=FILTER_IDS)
def test_host_build_equals_the_numpy_restatement_bit_for_bit(host, case):
    """Per frame and filter setting the numpy filters run once; every (s, t) and margin is then selected from those four filtered halves."""
    size, with_variance, iterations, (r, fr) = case
    a, b, va, vb, f = filter_set_inputs(case)
    fa, fb, na, nb = select_ref.filtered_halves(a, b, f, va, vb, iterations, r, fr)
    for s, t in RADII:
        for margin in MARGINS:
            got = host(a, b, f, va, vb, iterations=iterations, search_radius=r, patch_radius=fr, error_radius=s, blend_radius=t, margin=margin)
            want = select_ref.select(a, b, fa, fb, na, nb, s, t, margin)
            assert_same_outputs(got, want, (s, t, margin))


def test_zero_radii_and_the_margin_flag_are_the_stated_defaults(host):
    a, b, va, vb, f = inputs(11, 33, 18)
    default = host(a, b, f, va, vb)
    assert_same_outputs(default, host(a, b, f, va, vb, error_radius=5, blend_radius=2, margin=0.01))
    assert_same_outputs(default, select_ref.denoise_select(a, b, f, va, vb))
    # a margin of 0 is a margin of 0, not the default: on the synthetic frame at noise 0.3 it sends four times as much of the walls to non-local means
    a, b, f, _ = select_ref.synthetic_frame(0, noise=0.3)
    walls = (slice(None), slice(0, 28))
    assert host(a, b, f, margin=0.0)["blend"][walls].mean() > 2.0 * host(a, b, f)["blend"][walls].mean() > 0.0


@pytest.mark.parametrize("with_variance", [True, False], ids=["variance", "pair-variance"])
def test_the_extreme_margins_give_the_two_existing_filters(host, with_variance):
    """Against the host harnesses of the two filters themselves (tests/denoise_host, tests/nlm_host), loaded from their own libraries."""
    dh, nh = denoise_ref.host(), nlm_ref.host()
    check_composition(host, lambda c, v, f, it: dh(c, v, f, it)[0], nh, with_variance)


def test_a_nan_of_the_filter_that_was_not_chosen_stays_out(host):
    check_unchosen_nan_stays_out(host)


@pytest.mark.parametrize("with_variance", [True, False], ids=["variance", "pair-variance"])
def test_exchanging_the_halves_changes_no_output(host, with_variance):
    check_exchange(host, with_variance)


@pytest.mark.parametrize("with_variance", [True, False], ids=["variance", "pair-variance"])
def test_a_pixel_depends_on_the_stated_margin_of_pixels_around_it(host, with_variance):
    """At the defaults, 2 à-trous iterations: max(7 + 3 + 1, 6) + 5 + 2 = 18 pixels; a 45x43 crop of a 58x54 frame keeps an interior of 9x7."""
    a, b, va, vb, f = inputs(9, 58, 54, with_variance)
    check_locality(host, a, b, va, vb, f, (slice(4, 47), slice(6, 51)))
    # ... and where the à-trous reach is the larger one: r 1, f 1, s 1, t 1 -> max(3, 6) + 2 = 8
    check_locality(host, a, b, va, vb, f, (slice(4, 33), slice(6, 35)), error_radius=1, blend_radius=1, search_radius=1, patch_radius=1)


@pytest.mark.parametrize("seed", range(8))
def test_the_selection_sides_with_the_better_filter_where_the_truth_is_known(seed):
    """The 64x48 frame of select_ref.synthetic_frame, noise 0.15, everything at its default, 5 à-trous iterations, no variances, through the numpy
    path.  (A numpy prototype of this arithmetic: left MSE F 1.2e-5, N 3.7e-4, output about 3e-5, at most 0.37 of their geometric mean, mean beta
    0.05; right beta 1 everywhere, MSE F 0.06, N 0.002.  At noise 0.3 and margin 0 the estimator's power runs out — DESIGN.md section 10b.)"""
    a, b, f, truth = select_ref.synthetic_frame(seed)
    select_ref.check_synthetic(select_ref.denoise_select(a, b, f), truth)
