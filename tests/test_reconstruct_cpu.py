"""rttnw_reconstruct without a GPU: the host build of the arithmetic the device kernels run (rttnw_amd/csrc/reconstruct.hpp, built by
tests/reconstruct_host) against a tap-ordered numpy restatement of the contract in include/rttnw_hip.h — bit for bit, for every validity
pattern, with the invalid pixels poisoned — and the properties the contract promises."""
import numpy as np
import pytest

import denoise_cases
import denoise_ref
import reconstruct_ref


@pytest.fixture(scope="module")
def host():
    return reconstruct_ref.host()


@pytest.fixture(scope="module")
def denoise_host():
    return denoise_ref.host()


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _patterns(rng, w, h):
    yield "all", np.ones((h, w), dtype=bool)
    yield "none", np.zeros((h, w), dtype=bool)
    for level in (1, 2, 3):
        yield "lattice%d" % level, reconstruct_ref.lattice(w, h, level)
    yield "random10", rng.random((h, w)) < 0.1


def _poisoned(colour, var, valid):
    c = colour.copy()
    c[~valid] = np.nan
    v = None
    if var is not None:
        v = var.copy()
        v[~valid] = np.nan
    return c, v


@pytest.mark.parametrize("with_variance", [True, False], ids=["variance", "no-variance"])
@pytest.mark.parametrize("size", [(61, 47), (1, 1)], ids=["61x47", "1x1"])
def test_host_build_equals_the_numpy_restatement_bit_for_bit(host, size, with_variance):
    rng = np.random.default_rng(size[0] * 2 + int(with_variance))
    colour, var, f = denoise_ref.random_inputs(rng, size[0], size[1], with_variance)
    filled_something = False
    for name, valid in _patterns(rng, size[0], size[1]):
        c, v = _poisoned(colour, var, valid)
        for iterations in (0, 1, 5, 8):
            out, rgba, out_var, ok = host(c, v, valid, f, iterations)
            want, want_rgba, want_var, want_ok = reconstruct_ref.reconstruct(c, v, valid, f, iterations)
            assert np.array_equal(ok, want_ok), (name, iterations)
            assert _same_bits(out, want), (name, iterations)
            assert np.array_equal(rgba, want_rgba), (name, iterations)
            if with_variance:
                assert _same_bits(out_var, want_var), (name, iterations)
            else:
                assert out_var is None
            # a NaN of an invalid pixel reaches nothing (the inputs' own NaN variances stay in the variance output only)
            assert np.isfinite(out).all(), (name, iterations)
            assert set(np.unique(ok)) <= {0, 1}
            assert (rgba[..., 3] == 255 * ok).all() and (out[ok == 0] == 0.0).all() and (rgba[ok == 0] == 0).all()
            if with_variance:
                assert np.isposinf(out_var[ok == 0]).all()
            filled_something = filled_something or (iterations > 0 and (ok != 0).sum() > valid.sum() + (f["alpha"] == 0.0).sum())
    assert filled_something or size == (1, 1)


@pytest.mark.parametrize("with_variance", [True, False], ids=["variance", "no-variance"])
def test_every_pixel_valid_is_rttnw_denoise(host, denoise_host, with_variance):
    rng = np.random.default_rng(11 + int(with_variance))
    colour, var, f = denoise_ref.random_inputs(rng, 61, 47, with_variance)
    valid = np.ones((47, 61), dtype=np.uint8)
    for iterations in (0, 1, 5, 8):
        out, rgba, out_var, ok = host(colour, var, valid, f, iterations)
        assert (ok == 1).all()
        for want, want_rgba, want_var in (denoise_ref.denoise(colour, var, f, iterations), denoise_host(colour, var, f, iterations)):
            assert _same_bits(out, want), iterations
            assert np.array_equal(rgba, want_rgba)
            if with_variance:
                assert _same_bits(out_var, want_var), iterations
    # ... with the caller's sigmas too
    kw = dict(sigma_luminance=1.5, sigma_normal=8.0, sigma_depth=0.02)
    assert _same_bits(host(colour, var, valid, f, 3, **kw)[0], denoise_host(colour, var, f, 3, **kw)[0])
    assert not _same_bits(host(colour, var, valid, f, 3, **kw)[0], host(colour, var, valid, f, 3)[0])


def test_with_no_pixel_valid_only_the_background_comes_out(host):
    rng = np.random.default_rng(21)
    colour, var, f = denoise_ref.random_inputs(rng, 61, 47)
    sky = f["alpha"] == 0.0
    assert 50 < sky.sum() < sky.size
    nan = np.full_like(colour, np.nan)
    for iterations in (1, 5):
        out, rgba, out_var, ok = host(nan, nan, np.zeros(sky.shape, dtype=np.uint8), f, iterations)
        assert np.array_equal(ok != 0, sky)                    # a sky pixel is no tap: nothing spreads from it
        assert _same_bits(out[sky], f["albedo"][sky]) and (out_var[sky] == 0.0).all()
        assert (out[~sky] == 0.0).all() and np.isposinf(out_var[~sky]).all() and (rgba[~sky] == 0).all()
    out, rgba, out_var, ok = host(nan, nan, np.zeros(sky.shape, dtype=np.uint8), f, 0)      # 0 iterations: no background fill either
    assert (ok == 0).all() and (out == 0.0).all() and (rgba == 0).all() and np.isposinf(out_var).all()


def test_out_valid_is_monotone_in_the_iteration_count(host):
    rng = np.random.default_rng(31)
    colour, var, f = denoise_ref.random_inputs(rng, 61, 47)
    for valid in (reconstruct_ref.lattice(61, 47, 3), rng.random((47, 61)) < 0.02):
        c, v = _poisoned(colour, var, valid)
        before = valid.copy()
        counts = []
        for iterations in range(0, 9):
            ok = host(c, v, valid, f, iterations)[3] != 0
            assert (ok | ~before).all(), iterations             # whoever held a value still does
            before = ok
            counts.append(int(ok.sum()))
        assert counts[0] == valid.sum() and counts[-1] > 4 * counts[0]


def test_a_filled_pixel_takes_its_neighbours_value_and_variance(host):
    """A flat wall with one colour on the lattice: every pixel comes out with that colour, to rounding, and a filled pixel's variance is the
    weighted combination of its taps' — below theirs, never +inf where a tap had one."""
    h, w = 40, 48
    f = {"albedo": np.full((h, w, 3), 0.6), "normal": np.tile([0.0, 0.6, 0.8], (h, w, 1)), "depth": np.full((h, w), 9.0), "alpha": np.ones((h, w))}
    valid = reconstruct_ref.lattice(w, h, 2)
    colour = np.where(valid[..., None], [0.3, 0.9, 0.06], np.nan)
    var = np.where(valid[..., None], np.full((h, w, 3), 1e-2), np.nan)
    out, rgba, out_var, ok = host(colour, var, valid, f, 3)
    assert (ok == 1).all() and (rgba[..., 3] == 255).all()
    assert np.all(np.abs(out - [0.3, 0.9, 0.06]) <= 64 * np.spacing(1.0))
    assert np.isfinite(out_var).all() and (out_var < 1e-2).all() and (out_var > 0.0).all()
    # without a variance in any tap, the filled pixels' is +inf and stays that
    var_inf = np.where(valid[..., None], np.full((h, w, 3), np.inf), np.nan)
    _, _, out_var, ok = host(colour, var_inf, valid, f, 3)
    assert (ok == 1).all() and np.isposinf(out_var).all()


def test_nothing_is_filled_across_an_edge_between_orthogonal_normals(host):
    h, w = 32, 40
    left = np.zeros((h, w), dtype=bool)
    left[:, : w // 2] = True
    normal = np.where(left[..., None], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]) * np.ones((h, w, 1))
    f = {"albedo": np.full((h, w, 3), 0.5), "normal": normal, "depth": np.full((h, w), 10.0), "alpha": np.ones((h, w))}
    valid = left & reconstruct_ref.lattice(w, h, 1)             # values on the left wall only
    colour = np.where(valid[..., None], np.ones((h, w, 3)), np.nan)
    out, _, _, ok = host(colour, None, valid, f, 5)
    assert np.array_equal(ok != 0, left)                        # w_n = 0 exactly across the edge: the right wall holds nothing
    assert (out[~left] == 0.0).all() and np.all(np.abs(out[left] - 1.0) < 1e-12)


# ---- the frames and masks of tests/denoise_cases.py: what the device is held to in tests/test_gpu_reconstruct.py, anchored here without one

@pytest.mark.parametrize("size,with_variance", denoise_cases.FRAMES, ids=denoise_cases.FRAME_IDS)
def test_host_build_equals_the_numpy_restatement_on_hostile_frames(host, size, with_variance):
    """Every size, mask, iteration count and sigma set; every pixel of every output, the invalid pixels poisoned with NaN."""
    f = denoise_cases.frame(size, with_variance)[2]
    masks = denoise_cases.masked_frames(size, with_variance)
    assert list(masks) == denoise_cases.MASK_IDS
    for name, (c, v, valid) in masks.items():
        assert np.isnan(c[~valid]).all() and (v is None or np.isnan(v[~valid]).all())
        for iterations in denoise_cases.ITERATIONS:
            for k, sigmas in enumerate(denoise_cases.SIGMAS):
                got = host(c, v, valid, f, iterations, **sigmas)
                want = denoise_cases.reconstruct_reference(size, with_variance, name, iterations, k)
                denoise_cases.assert_same_results(got, want, (name, iterations, k))
                assert np.isfinite(got[0]).all(), (name, iterations, k)             # a NaN of an invalid pixel reaches nothing


def test_the_sparse_mask_reaches_every_branch_of_the_fill():
    """45x37 with 2 pixels in 100 valid, 5 passes, on the restatement's output: pixels filled from their taps, pixels never filled (a zero normal,
    or nothing in reach), and filled pixels none of whose taps had a finite variance (theirs is +inf).  Measured: 1294, 58 and 18."""
    filled, never, no_variance = denoise_cases.fill_counts((45, 37), True, "random0.02", 5)
    print("filled %d, never filled %d, filled with no finite-variance tap %d" % (filled, never, no_variance))
    assert filled > 0 and never > 0 and no_variance > 0
