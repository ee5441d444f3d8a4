"""rttnw_svgf_push without a GPU: the host build of the arithmetic the device kernels run (rttnw_amd/csrc/svgf.hpp and the headers it composes,
built by tests/svgf_host) against the contract of include/rttnw_hip.h restated as a composition of the three stages' restatements — bit for
bit, every output, along chains of three calls that start from a made-up history — and the four properties the contract promises, on the
restatement and on the host build: agreement with the existing chain, textured albedo, noisy frames, feedback depth."""
import numpy as np
import pytest

import denoise_ref
import svgf_ref
import variance_ref
from svgf_cases import (CASE_IDS, CASES, chain, check_agreement_with_the_existing_chain, check_chain, check_feedback_depth, check_noisy_frames,
                        check_textured_albedo, first_frame, settings)

IMPLEMENTATIONS = [svgf_ref.Restated, svgf_ref.Host]
IDS = ["restatement", "host-build"]


def test_the_cases_cover_what_they_claim():
    assert len(CASES) == 72 and {(c[1], c[2]) for c in CASES} == {(fb, dm) for fb in (0, 1, 2) for dm in (0, 1)}
    bad = sum(1 for c in CASES if c[0][6])
    assert len(CASES) // 6 <= bad <= len(CASES) // 3, bad                  # about a quarter hold NaN and inf
    assert {c[0][0] for c in CASES} == {(1, 1), (3, 5), (37, 29), (70, 41)}


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_host_build_equals_the_restatement_bit_for_bit(case):
    check_chain(svgf_ref.Host, svgf_ref.Restated, case)


@pytest.mark.parametrize("case", CASES[-6:], ids=CASE_IDS[-6:])
def test_a_chain_from_an_empty_state_agrees_too(case):
    """What the device's handle can be given: no loaded state, the made-up history pushed as a first frame."""
    check_chain(svgf_ref.Host, svgf_ref.Restated, case, loaded=False)


def test_the_feedback_reaches_the_next_frame_and_only_the_colour():
    """Feedback changes the accumulation from the second call on, and never the moments, the estimate, length or prev_xy."""
    case0, case1 = (CASES[-1][0], 0, 0), (CASES[-1][0], 1, 0)
    (w, h) = case0[0][0]
    a, b = svgf_ref.Host(w, h, **settings(case0)), svgf_ref.Host(w, h, **settings(case1))
    for k, (lin, f, cam) in enumerate([first_frame(case0)] + chain(case0)[1]):
        x, y = a.push(lin, f, cam), b.push(lin, f, cam)
        for name in ("moment1_rgb", "moment2_rgb", "variance_rgb", "length", "prev_xy"):
            assert np.array_equal(x[name], y[name], equal_nan=True), (name, k)
        assert np.array_equal(x["accumulated_rgb"], y["accumulated_rgb"], equal_nan=True) == (k == 0), k


@pytest.mark.parametrize("make", IMPLEMENTATIONS, ids=IDS)
def test_agreement_with_the_existing_chain(make):
    check_agreement_with_the_existing_chain(make, variance_ref.estimate, denoise_ref.denoise)


@pytest.mark.parametrize("make", IMPLEMENTATIONS, ids=IDS)
def test_textured_albedo(make):
    check_textured_albedo(make)


@pytest.mark.parametrize("make", IMPLEMENTATIONS, ids=IDS)
def test_noisy_frames(make):
    print("mean squared deviation of accumulated_rgb from 0.5 at frame 8 (feedback 0, feedback 1):", check_noisy_frames(make))


@pytest.mark.parametrize("make", IMPLEMENTATIONS, ids=IDS)
def test_feedback_depth(make):
    check_feedback_depth(make)
