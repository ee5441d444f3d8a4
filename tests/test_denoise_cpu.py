"""rttnw_denoise without a GPU: the host build of the arithmetic the device kernels run (rttnw_amd/csrc/denoise.hpp, built by
tests/denoise_host) against a tap-ordered numpy restatement of the contract in include/rttnw_hip.h — bit for bit — and the properties
the contract promises."""
import numpy as np
import pytest

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
    rng = np.random.default_rng(1)
    colour, var, f = denoise_ref.random_inputs(rng, 37, 29)
    out, rgba, out_var = host(colour, var, f, 0)
    assert _same_bits(out, colour) and _same_bits(out_var, var)
    assert np.array_equal(rgba, denoise_ref.quantise(colour))


def test_a_constant_image_stays_constant(host):
    h, w = 48, 40
    f = {"albedo": np.full((h, w, 3), 0.73), "normal": np.tile([0.0, 0.6, 0.8], (h, w, 1)), "depth": np.full((h, w), 12.5),
         "alpha": np.ones((h, w))}
    colour = np.tile([0.31, 1.7, 0.052], (h, w, 1))
    var = np.full((h, w, 3), 1e-3)
    for v in (None, var):
        out, _, _ = host(colour, v, f, 5)
        # 25 taps of normalised weights: the sum of w c over the sum of w, each within a few ulp of c
        assert np.all(np.abs(out - colour) <= 32 * np.spacing(colour)), np.abs(out - colour).max()


def test_alpha_zero_pixels_pass_through_and_reach_no_neighbour(host):
    rng = np.random.default_rng(2)
    colour, var, f = denoise_ref.random_inputs(rng, 37, 29)
    sky = f["alpha"] == 0.0
    assert sky.sum() > 50
    out, _, out_var = host(colour, var, f, 4)
    assert _same_bits(out[sky], colour[sky]) and _same_bits(out_var[sky], var[sky])
    other = colour.copy()
    other[sky] = rng.exponential(50.0, size=(int(sky.sum()), 3))
    f2 = dict(f, albedo=f["albedo"].copy(), normal=f["normal"].copy(), depth=f["depth"].copy())
    f2["albedo"][sky], f2["normal"][sky], f2["depth"][sky] = 0.9, [0.0, 0.0, 1.0], 5.0
    out2, _, _ = host(other, var, f2, 4)
    assert _same_bits(out2[~sky], out[~sky])
    assert _same_bits(out2[sky], other[sky])


def test_no_colour_crosses_an_edge_between_orthogonal_normals(host):
    rng = np.random.default_rng(3)
    h, w = 40, 48
    left = np.zeros((h, w), dtype=bool)
    left[:, : w // 2] = True
    normal = np.where(left[..., None], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]) * np.ones((h, w, 1))
    f = {"albedo": np.full((h, w, 3), 0.5), "normal": normal, "depth": np.full((h, w), 10.0), "alpha": np.ones((h, w))}
    colour = rng.exponential(1.0, size=(h, w, 3))
    out, _, _ = host(colour, None, f, 5)
    other = colour.copy()
    other[~left] += 100.0
    out2, _, _ = host(other, None, f, 5)
    assert _same_bits(out2[left], out[left])                       # w_n = 0 exactly across the edge
    assert np.all(out2[~left] > 90.0) and np.all(out[left] < 20.0)
    assert out[left].std() < 0.5 * colour[left].std()              # ... while each side was smoothed


def test_a_variance_that_is_not_finite_is_treated_as_absent(host):
    rng = np.random.default_rng(4)
    colour, _, f = denoise_ref.random_inputs(rng, 37, 29, with_variance=False)
    plain, _, _ = host(colour, None, f, 3)
    for bad in (np.inf, np.nan):
        out, _, out_var = host(colour, np.full(colour.shape, bad), f, 3)
        assert _same_bits(out, plain)
        assert not np.isfinite(out_var).any()
    # one pixel without a variance among pixels that have one: it is filtered with w_l = 1, and keeps its own variance
    var = np.full(colour.shape, 0.04)
    var[10, 10] = np.inf
    f1 = dict(f, alpha=np.ones_like(f["alpha"]))
    out, _, out_var = host(colour, var, f1, 1)
    want, _, want_var = denoise_ref.denoise(colour, var, f1, 1)
    assert _same_bits(out, want) and _same_bits(out_var, want_var)
    assert np.isinf(out_var[10, 10]).all() and np.isfinite(out_var[10, 11]).all()
