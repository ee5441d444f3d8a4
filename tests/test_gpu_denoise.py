"""rttnw_denoise on the MI355X: the device kernels equal the host build of the same header (tests/denoise_host) bit for bit on real
renders, and the filter lowers the error against the CPU oracle's converged windows — the reference's restatement, never ourselves."""
import numpy as np
import pytest

import denoise_cases
import denoise_ref
from golden_cases import WINDOWS, load_windows
from rttnw_amd import abi, library, render
from rttnw_amd import scene as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    return denoise_ref.host()


@pytest.fixture(scope="module")
def scenes(gpu):
    lib = library.scenes()
    return {name: S.build(gpu, lib, name, S.load_earth() if name == "final_scene" else None) for name in ("cornell_box", "final_scene")}


def _frame(scenes, name, w, spp, adaptive):
    """(linear, stderr or None, features) of a frame: a plain render, or an adaptive one that runs to its cap and reports its noise."""
    sc, setup = scenes[name]
    cam, p = S.params_for(setup, w, w, spp, precision=abi.F64)
    if adaptive:
        lin, _, n, se, _ = render.render_adaptive(sc, cam, p, pass_spp=spp, rel_error=0.0)
        assert (n == spp).all()
    else:
        lin, _, _ = render.render_host(sc, cam, p)
        se = None
    return lin, se, render.render_features(sc, cam, p)


@pytest.mark.parametrize("adaptive", [True, False], ids=["variance", "no-variance"])
@pytest.mark.parametrize("name", ["cornell_box", "final_scene"])
def test_device_equals_host_harness(scenes, host, name, adaptive):
    lin, se, f = _frame(scenes, name, 128, 16, adaptive)
    var = None if se is None else np.square(se)
    for iterations in (5, 1, 0):
        out, rgba, out_var = render.denoise(lin, f, se, iterations=iterations)
        want, want_rgba, want_var = host(lin, var, f, iterations)
        assert np.array_equal(out.view(np.uint64), want.view(np.uint64)), (iterations, np.nanmax(np.abs(out - want)))
        assert np.array_equal(rgba, want_rgba)
        if adaptive:
            assert np.array_equal(out_var.view(np.uint64), want_var.view(np.uint64)), iterations
        else:
            assert out_var is None
    assert np.array_equal(render.denoise(lin, f, se, iterations=0)[0], lin)
    # explicit parameters travel to the kernels
    out, _, _ = render.denoise(lin, f, se, iterations=3, sigma_luminance=2.0, sigma_normal=16.0, sigma_depth=0.03)
    want, _, _ = host(lin, var, f, 3, 2.0, 16.0, 0.03)
    assert np.array_equal(out.view(np.uint64), want.view(np.uint64))


def _window_errors(scenes, name, adaptive):
    """Per committed oracle window of the 800x800 frame: (key, MSE of the 16-spp render, MSE of its denoised image)."""
    lin, se, f = _frame(scenes, name, 800, 16, adaptive)
    out, _, _ = render.denoise(lin, f, se)
    gold = load_windows()
    rows = []
    for key, scene, w, h, spp, x0, y0, cw, ch, _ in WINDOWS:
        if scene != name or not key.startswith("t2_"):
            continue
        ref = gold[key + "_linear"]
        crop = (slice(y0, y0 + ch), slice(x0, x0 + cw))
        rows.append((key, float(np.mean((lin[crop] - ref) ** 2)), float(np.mean((out[crop] - ref) ** 2))))
    return rows


@pytest.mark.parametrize("adaptive", [True, False], ids=["variance", "no-variance"])
def test_denoising_lowers_the_error_against_the_oracle(scenes, adaptive):
    """cornell_box 800x800 spp 16, default parameters, against the oracle's windows at spp 1000 (tests/golden/golden_windows.npz): the
    denoised image is closer to the converged one than the render it was made from, in every window.  Measured (MSE noisy / denoised):
    with the variance input 31.2, 29.3, 26.2 in t2_cornell_0..2; without it 44.3, 53.1, 53.5."""
    rows = _window_errors(scenes, "cornell_box", adaptive)
    assert [r[0] for r in rows] == ["t2_cornell_0", "t2_cornell_1", "t2_cornell_2"]
    for key, noisy, den in rows:
        print("%s %s: MSE noisy %.4g, denoised %.4g, ratio %.2f" % (key, "variance" if adaptive else "no variance", noisy, den, noisy / den))
    for key, noisy, den in rows:
        assert den < noisy, (key, noisy, den)


@pytest.mark.parametrize("adaptive", [True, False], ids=["variance", "no-variance"])
def test_final_scene_windows_are_recorded(scenes, adaptive):
    """final_scene's four windows — earth and the blue medium, the glass sphere, the noise sphere, the sphere cluster: where a filter guided
    by the FIRST hit is expected to be weakest (what lies behind glass, what a mirror shows, is not in its features).  Recorded, not
    asserted (profiles/LEDGER.md); the run only has to be finite.  Measured (MSE noisy / denoised): with the
    variance input 11.4, 16.0, 6.5, 8.4 in t2_final_0..3; without it 34.6, 35.9, 5.7, 3.7."""
    rows = _window_errors(scenes, "final_scene", adaptive)
    assert len(rows) == 4
    for key, noisy, den in rows:
        print("%s %s: MSE noisy %.4g, denoised %.4g, ratio %.2f" % (key, "variance" if adaptive else "no variance", noisy, den, noisy / den))
        assert np.isfinite(noisy) and np.isfinite(den)


# ---- the frames of tests/denoise_cases.py: sizes no render here has, values no render has, all eight passes

def _device(colour, variance, f, iterations, **sigmas):
    """rttnw_denoise as a `run` of tests/denoise_cases.py: the variance as it stands, so an infinite, a NaN and a zero one arrive exactly."""
    return render.denoise(colour, f, iterations=iterations, variance=variance, **sigmas)


@pytest.mark.parametrize("size,with_variance", denoise_cases.FRAMES, ids=denoise_cases.FRAME_IDS)
def test_device_equals_restatement_and_host_harness_on_hostile_frames(gpu, host, size, with_variance):
    """Every size, iteration count and sigma set of tests/denoise_cases.py; every pixel of the linear image, its RGBA8 and its variance, against
    the numpy restatement and against the host build."""
    denoise_cases.assert_not_vacuous(size, with_variance)
    colour, var, f = denoise_cases.frame(size, with_variance)
    for iterations in denoise_cases.ITERATIONS:
        for k, sigmas in enumerate(denoise_cases.SIGMAS):
            got = _device(colour, var, f, iterations, **sigmas)
            denoise_cases.assert_same_results(got, denoise_cases.denoise_reference(size, with_variance, iterations, k), (iterations, k))
            denoise_cases.assert_same_results(got, host(colour, var, f, iterations, **sigmas), (iterations, k, "host"))
            assert (got[2] is None) == (not with_variance)


@pytest.mark.parametrize("check", denoise_cases.PROPERTIES, ids=[c.__name__[6:] for c in denoise_cases.PROPERTIES])
def test_the_contract_properties_hold_on_the_device(gpu, check):
    check(_device)


def test_passes_6_to_8_change_the_image_and_the_farthest_tap_weighs(gpu):
    """129x7: eight iterations are not five — the passes whose stride exceeds most of the frame still run —, and the one tap of pass 8 that lies
    inside the image (column 0 to column 128, row 0 to row 128 of 7x129) is neither dropped nor wrapped: bit for bit the restatement, in which
    it weighs."""
    for with_variance in (True, False):
        colour, var, f = denoise_cases.frame((129, 7), with_variance)
        five, eight = (_device(colour, var, f, it)[0] for it in (5, 8))
        assert not denoise_cases.same(five, eight)
        assert denoise_cases.same(eight, denoise_cases.denoise_reference((129, 7), with_variance, 8, 0)[0])
    denoise_cases.check_far_tap(_device)
    denoise_cases.check_far_tap(_device, transposed=True)


@pytest.mark.parametrize("with_variance", [True, False], ids=["variance", "no-variance"])
def test_a_pixel_depends_on_the_stated_margin_of_pixels_around_it(gpu, with_variance):
    """A 53x33 crop of the 70x41 frame, its origin (5, 3) off the 32x8 blocks, 2 iterations: 6 pixels in from the crop's edge every pixel is the
    whole frame's, bit for bit; 5 pixels in it is not (tests/denoise_cases.py says why 6; tests/test_denoise_cpu.py holds the host build and the
    restatement to both halves)."""
    denoise_cases.check_locality(_device, with_variance)
