"""rttnw_denoise without a GPU: the host build of the arithmetic the device kernels run (rttnw_amd/csrc/denoise.hpp, built by
tests/denoise_host) against a tap-ordered numpy restatement of the contract in include/rttnw_hip.h — bit for bit — and the properties
the contract promises."""
import numpy as np
import pytest

import denoise_cases
import denoise_ref


@pytest.fixture(scope="module")
def host():
    return denoise_ref.host()


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("with_variance", [True, False])
@pytest.mark.parametrize("size", [(37, 29), (64, 64)])
def test_host_build_equals_the_numpy_restatement_bit_for_bit(host, size, with_variance):
    rng = np.random.default_rng(size[0] * 2 + int(with_variance))
    colour, var, f = denoise_ref.random_inputs(rng, size[0], size[1], with_variance)
    for iterations in range(1, 6):
        out, rgba, out_var = host(colour, var, f, iterations)
        want, want_rgba, want_var = denoise_ref.denoise(colour, var, f, iterations)
        assert _same_bits(out, want), (iterations, np.nanmax(np.abs(out - want)))
        assert np.array_equal(rgba, want_rgba)
        if with_variance:
            assert _same_bits(out_var, want_var), iterations
        assert not np.array_equal(out, colour)                     # ... and it did filter something


def test_explicit_sigmas_reach_the_weights(host):
    rng = np.random.default_rng(5)
    colour, var, f = denoise_ref.random_inputs(rng, 40, 33)
    kw = dict(sigma_luminance=1.5, sigma_normal=8.0, sigma_depth=0.02)
    out, _, out_var = host(colour, var, f, 3, **kw)
    want, _, want_var = denoise_ref.denoise(colour, var, f, 3, **kw)
    assert _same_bits(out, want) and _same_bits(out_var, want_var)
    assert not _same_bits(out, host(colour, var, f, 3)[0])


def test_zero_iterations_is_the_identity(host):
    denoise_cases.check_zero_iterations_is_the_identity(host)


def test_a_constant_image_stays_constant(host):
    denoise_cases.check_a_constant_image_stays_constant(host)


def test_alpha_zero_pixels_pass_through_and_reach_no_neighbour(host):
    denoise_cases.check_alpha_zero_pixels_pass_through_and_reach_no_neighbour(host)


def test_no_colour_crosses_an_edge_between_orthogonal_normals(host):
    denoise_cases.check_no_colour_crosses_an_edge_between_orthogonal_normals(host)


def test_a_variance_that_is_not_finite_is_treated_as_absent(host):
    denoise_cases.check_a_variance_that_is_not_finite_is_treated_as_absent(host)


# ---- the frames of tests/denoise_cases.py: what the device is held to in tests/test_gpu_denoise.py, anchored here without one

@pytest.mark.parametrize("size,with_variance", denoise_cases.FRAMES, ids=denoise_cases.FRAME_IDS)
def test_hostile_frames_hold_every_kind_of_value(size, with_variance):
    """From the inputs alone: every frame of 297 pixels or more has hit pixels with a zero normal, a negative and a zero depth, fractional alpha, an
    albedo channel in (0, 1e-3] and one below the threshold beside one above it, pixels with alpha 0, and each of an infinite, a NaN and a zero
    variance."""
    counts = denoise_cases.assert_not_vacuous(size, with_variance)
    assert len(counts) == (10 if with_variance else 7)
    colour, var, f = denoise_cases.frame(size, with_variance)
    assert colour.shape == (size[1], size[0], 3) and f["depth"].shape == (size[1], size[0])


@pytest.mark.parametrize("size,with_variance", denoise_cases.FRAMES, ids=denoise_cases.FRAME_IDS)
def test_host_build_equals_the_numpy_restatement_on_hostile_frames(host, size, with_variance):
    """Every size, iteration count (up to the 8 the entry point allows: strides beyond the frame) and sigma set; every pixel of every output."""
    colour, var, f = denoise_cases.frame(size, with_variance)
    for iterations in denoise_cases.ITERATIONS:
        for k, sigmas in enumerate(denoise_cases.SIGMAS):
            got = host(colour, var, f, iterations, **sigmas)
            denoise_cases.assert_same_results(got, denoise_cases.denoise_reference(size, with_variance, iterations, k), (iterations, k))
            assert (got[2] is None) == (not with_variance)


def test_passes_6_to_8_change_the_image_and_the_farthest_tap_weighs(host):
    for with_variance in (True, False):
        five, eight = (denoise_cases.denoise_reference((129, 7), with_variance, it, 0)[0] for it in (5, 8))
        assert not denoise_cases.same(five, eight)
    denoise_cases.check_far_tap(host)
    denoise_cases.check_far_tap(host, transposed=True)


@pytest.mark.parametrize("with_variance", [True, False])
def test_a_pixel_depends_on_the_stated_margin_of_pixels_around_it(host, with_variance):
    denoise_cases.check_locality(host, with_variance)
    denoise_cases.check_locality(denoise_ref.denoise, with_variance)
