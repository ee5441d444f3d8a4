"""rttnw_reconstruct on the MI355X: the device kernels equal the host build of the same header (tests/reconstruct_host) bit for bit on real
renders of which only a lattice holds a value — the rest poisoned with NaN — and, with every pixel valid, equal rttnw_denoise."""
import numpy as np
import pytest

import denoise_cases
import reconstruct_ref
from rttnw_amd import abi, library, render
from rttnw_amd import scene as S

pytestmark = pytest.mark.gpu
SIZES = [(96, 96), (45, 37)]           # 45x37: no multiple of the 8x8 tiles nor of the 32x8 launch blocks; its level-6 lattice is one pixel
LEVELS = (0, 1, 2, 3, 6)
SPP = 16


@pytest.fixture(scope="module")
def host():
    return reconstruct_ref.host()


@pytest.fixture(scope="module")
def scenes(gpu):
    lib = library.scenes()
    return {name: S.build(gpu, lib, name, S.load_earth() if name == "final_scene" else None) for name in ("cornell_box", "final_scene")}


@pytest.fixture(scope="module")
def frames(scenes):
    """(linear, stderr, features) of a frame: an adaptive render that runs to its cap and reports its noise.  Computed once per frame, read-only."""
    cache = {}

    def get(name, size):
        if (name, size) not in cache:
            sc, setup = scenes[name]
            cam, p = S.params_for(setup, size[0], size[1], SPP, precision=abi.F64)
            lin, _, n, se, _ = render.render_adaptive(sc, cam, p, pass_spp=SPP, rel_error=0.0)
            f = render.render_features(sc, cam, p)
            for a in (lin, se, f["albedo"], f["normal"], f["depth"], f["alpha"]):
                a.setflags(write=False)
            cache[(name, size)] = (lin, se, f)
        return cache[(name, size)]
    return get


def _bits(a):
    return a.view(np.uint64)


@pytest.mark.parametrize("with_variance", [True, False], ids=["variance", "no-variance"])
@pytest.mark.parametrize("size", SIZES, ids=["96x96", "45x37"])
@pytest.mark.parametrize("name", ["cornell_box", "final_scene"])
def test_device_equals_host_harness(frames, host, name, size, with_variance):
    lin, se, f = frames(name, size)
    filled = 0
    for level in LEVELS:
        valid = render.lattice_mask(size[0], size[1], level) != 0
        c = np.where(valid[..., None], lin, np.nan)
        s = np.where(valid[..., None], se, np.nan) if with_variance else None
        var = None if s is None else np.square(s)
        for iterations in (5, 1, 0):
            out, rgba, out_var, ok = render.reconstruct(c, valid, f, s, iterations=iterations)
            want, want_rgba, want_var, want_ok = host(c, var, valid, f, iterations)
            assert np.array_equal(ok, want_ok), (level, iterations)
            assert np.array_equal(_bits(out), _bits(want)), (level, iterations, np.nanmax(np.abs(out - want)))
            assert np.array_equal(rgba, want_rgba), (level, iterations)
            if with_variance:
                assert np.array_equal(_bits(out_var), _bits(want_var)), (level, iterations)
            else:
                assert out_var is None
            assert np.isfinite(out).all() and (rgba[..., 3] == 255 * ok).all()
            if iterations == 0:
                assert np.array_equal(ok != 0, valid) and np.array_equal(out[valid], lin[valid]) and (out[~valid] == 0.0).all()
            if iterations == 5 and 1 <= level <= 3:
                filled += int(ok.sum()) - int(valid.sum())
    assert filled > 0          # ... and pixels that held nothing came out holding a value
    # explicit parameters travel to the kernels
    valid = render.lattice_mask(size[0], size[1], 1) != 0
    c = np.where(valid[..., None], lin, np.nan)
    out = render.reconstruct(c, valid, f, None, iterations=3, sigma_luminance=2.0, sigma_normal=16.0, sigma_depth=0.03)[0]
    want = host(c, None, valid, f, 3, 2.0, 16.0, 0.03)[0]
    assert np.array_equal(_bits(out), _bits(want))
    assert not np.array_equal(_bits(out), _bits(render.reconstruct(c, valid, f, None, iterations=3)[0]))


@pytest.mark.parametrize("with_variance", [True, False], ids=["variance", "no-variance"])
@pytest.mark.parametrize("size", SIZES, ids=["96x96", "45x37"])
@pytest.mark.parametrize("name", ["cornell_box", "final_scene"])
def test_every_pixel_valid_is_rttnw_denoise(frames, name, size, with_variance):
    lin, se, f = frames(name, size)
    s = se if with_variance else None
    valid = np.ones((size[1], size[0]), dtype=np.uint8)
    for iterations in (5, 1, 0):
        out, rgba, out_var, ok = render.reconstruct(lin, valid, f, s, iterations=iterations)
        want, want_rgba, want_var = render.denoise(lin, f, s, iterations=iterations)
        assert (ok == 1).all()
        assert np.array_equal(_bits(out), _bits(want)) and np.array_equal(rgba, want_rgba), iterations
        if with_variance:
            assert np.array_equal(_bits(out_var), _bits(want_var)), iterations
        else:
            assert out_var is None and want_var is None


# ---- the frames and masks of tests/denoise_cases.py: sizes, values and validity patterns no render here has, all eight passes

@pytest.mark.parametrize("size,with_variance", denoise_cases.FRAMES, ids=denoise_cases.FRAME_IDS)
def test_device_equals_restatement_and_host_harness_on_hostile_frames(gpu, host, size, with_variance):
    """Every size, mask, iteration count and sigma set of tests/denoise_cases.py; every pixel of the linear image, its RGBA8, its variance and
    out_valid, against the numpy restatement and against the host build.  The variance travels as it stands (`variance=`)."""
    f = denoise_cases.frame(size, with_variance)[2]
    for name, (c, v, valid) in denoise_cases.masked_frames(size, with_variance).items():
        for iterations in denoise_cases.ITERATIONS:
            for k, sigmas in enumerate(denoise_cases.SIGMAS):
                got = render.reconstruct(c, valid, f, iterations=iterations, variance=v, **sigmas)
                want = denoise_cases.reconstruct_reference(size, with_variance, name, iterations, k)
                denoise_cases.assert_same_results(got, want, (name, iterations, k))
                denoise_cases.assert_same_results(got, host(c, v, valid, f, iterations, **sigmas), (name, iterations, k, "host"))
                assert np.isfinite(got[0]).all() and (got[2] is None) == (not with_variance)
    if size == (45, 37) and with_variance:
        assert min(denoise_cases.fill_counts(size, True, "random0.02", 5)) > 0          # filled, never filled, filled without a variance


def test_stderr_and_variance_are_one_input(gpu):
    colour, var, f = denoise_cases.frame((33, 9), False)
    stderr = np.full(colour.shape, 0.25)
    valid = denoise_cases.masked_frames((33, 9), False)["random0.3"][2]
    denoise_cases.assert_same_results(render.reconstruct(colour, valid, f, stderr, iterations=2),
                                      render.reconstruct(colour, valid, f, iterations=2, variance=np.square(stderr)))
    with pytest.raises(ValueError):
        render.reconstruct(colour, valid, f, stderr, variance=np.square(stderr))
