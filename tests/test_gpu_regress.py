"""rttnw_denoise_regress on the MI355X: the device kernels equal the host build of the same header (tests/regress_host) bit for bit in every
output, on synthetic frames that cross the kernel's tiles under both of its tile sizes and on real half renders with their feature maps; with
no regressor and no demodulation the call is rttnw_denoise_nlm; the exchange of the halves and locality hold on the device; the filter lowers
the error against the CPU oracle's converged windows — never against ourselves; the command line writes what the Python composition computes."""
import os
import subprocess
import sys

import numpy as np
import pytest

import regress_ref
from golden_cases import WINDOWS, load_windows
from nlm_cases import same_bits
from regress_cases import GPU_FRAMES, GPU_MASKS, GPU_RADII, assert_same_outputs, inputs, locality, swapped_equal
from rttnw_amd import abi, library, render
from rttnw_amd import scene as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host():
    return regress_ref.host()


@pytest.fixture(scope="module")
def scenes(gpu):
    lib = library.scenes()
    return {name: S.build(gpu, lib, name, S.load_earth() if name == "final_scene" else None) for name in ("cornell_box", "final_scene")}


def _frame(scenes, name, w, spp=16):
    """(half_a, half_b, features) of a frame: two plain renders of spp / 2 samples over disjoint sample ranges and the first-hit features of spp."""
    sc, setup = scenes[name]
    cam, p = S.params_for(setup, w, w, spp, precision=abi.F64)
    (a, _, _), (b, _, _) = render.render_halves(sc, cam, p)
    return a, b, render.render_features(sc, cam, p)


@pytest.fixture(scope="module")
def renders96(scenes):
    return {name: _frame(scenes, name, 96) for name in ("cornell_box", "final_scene")}


def _device(a, b, va, vb, features, **kw):
    return render.denoise_regress(a, b, va, vb, features, **kw)


@pytest.mark.parametrize("radii", GPU_RADII, ids=lambda rf: "r%d-f%d" % rf)
@pytest.mark.parametrize("size", GPU_FRAMES, ids=lambda s: "%dx%d" % s)
def test_device_equals_host_harness_on_frames_that_cross_the_tiles(gpu, host, size, radii):
    """Every output, bit for bit: masks 0, 1 and 4 run the 32-pixel tile at (1, 1) and (7, 3), mask 7 and everything at (16, 4) the 16-pixel tile;
    1x1 and 3x5 are all halo."""
    for with_variance in (True, False):
        a, b, va, vb, f = inputs(size[0] * 64 + radii[0] * 2 + int(with_variance), size[0], size[1], with_variance)
        for mask in GPU_MASKS:
            for demodulate in (False, True):
                kw = dict(mask=mask, demodulate=demodulate, search_radius=radii[0], patch_radius=radii[1])
                assert_same_outputs(_device(a, b, va, vb, f, **kw), host(a, b, va, vb, f, **kw), (size, radii, mask, demodulate, with_variance))


@pytest.mark.parametrize("name", ["cornell_box", "final_scene"])
def test_device_equals_host_harness_on_real_half_renders(renders96, host, name):
    a, b, f = renders96[name]
    for kw in ({}, dict(search_radius=10, patch_radius=3, k=0.45, ridge=1e-1)):
        got = _device(a, b, None, None, f, **kw)
        assert_same_outputs(got, host(a, b, None, None, f, **kw), (name, kw))
        assert np.isfinite(got["linear"]).all() and not np.array_equal(got["linear"], (a + b) * 0.5)
        assert set(np.unique(got["fit"])) <= {0.0, 1.0, 2.0} and (got["fit"] == 2.0).any()


@pytest.mark.parametrize("with_variance", [True, False], ids=["variance", "pair-variance"])
def test_no_regressor_and_no_demodulation_is_non_local_means_on_a_synthetic_frame(gpu, with_variance):
    """Property 1 against rttnw_denoise_nlm on the device, with the feature arrays NULL."""
    a, b, va, vb, _ = inputs(21, 37, 29, with_variance)
    for r, f, k in ((0, 0, 0.0), (16, 4, 0.45)):
        ours = render.denoise_regress(a, b, va, vb, None, mask=0, demodulate=False, search_radius=r, patch_radius=f, k=k)
        theirs = render.denoise_nlm(a, b, va, vb, search_radius=r, patch_radius=f, k=k)
        for name in ("linear", "rgba8", "half_a", "half_b", "error"):
            assert same_bits(ours[name], theirs[name]), (name, r, f)
        assert (ours["fit"] == 2.0).all()


def test_no_regressor_and_no_demodulation_is_non_local_means_on_final_scene(renders96):
    a, b, f = renders96["final_scene"]
    theirs = render.denoise_nlm(a, b)
    for features in (None, f):                                      # NULL feature arrays, and arrays that must not be read
        ours = render.denoise_regress(a, b, None, None, features, mask=0, demodulate=False)
        for name in ("linear", "rgba8", "half_a", "half_b", "error"):
            assert same_bits(ours[name], theirs[name]), name


def test_exchange_and_locality_on_final_scene(renders96):
    """Properties 2 and 3 at the defaults, the crop's origin and size off the tile grid (tests/test_regress_cpu.py says why the short margin is
    r + f: the pair variance's 3x3 reaches one pixel past the guides)."""
    a, b, f = renders96["final_scene"]
    swapped_equal(_device(a, b, None, None, f), _device(b, a, None, None, f))
    r, fr = regress_ref.DEFAULTS["search_radius"], regress_ref.DEFAULTS["patch_radius"]
    locality(_device, a, b, None, None, f, (slice(10, 75), slice(21, 90)), r, fr, r + fr)


def _window_errors(scenes, name):
    """Per committed oracle window of the 800x800 frame, halves of 8 samples, default parameters: (key, MSE of (a + b) / 2, of rttnw_denoise of that
    mean, of rttnw_denoise_nlm, of the regression without and with demodulation, share of pixels with fit < 2 in the last)."""
    a, b, f = _frame(scenes, name, 800)
    mean = (a + b) * 0.5
    guided, _, _ = render.denoise(mean, f)
    nlm = render.denoise_nlm(a, b)["linear"]
    plain = render.denoise_regress(a, b, None, None, f, demodulate=False)
    demod = render.denoise_regress(a, b, None, None, f)
    gold = load_windows()
    rows = []
    for key, scene, w, h, spp, x0, y0, cw, ch, _ in WINDOWS:
        if scene != name or not key.startswith("t2_"):
            continue
        ref = gold[key + "_linear"]
        crop = (slice(y0, y0 + ch), slice(x0, x0 + cw))
        rows.append((key,) + tuple(float(np.mean((img[crop] - ref) ** 2)) for img in (mean, guided, nlm, plain["linear"], demod["linear"])) +
                    (float((demod["fit"][crop] < 2.0).mean()),))
    for key, noisy, den, nl, reg, reg_d, unfit in rows:
        print("%s: MSE plain 16 spp %.4g, rttnw_denoise %.4g, rttnw_denoise_nlm %.4g, regress without demodulation %.4g, with %.4g (%.1fx plain, "
              "%.2fx rttnw_denoise, %.2fx nlm), fit < 2 on %.2f %% of the pixels" % (key, noisy, den, nl, reg, reg_d, noisy / reg_d, den / reg_d, nl / reg_d,
                                                                                100.0 * unfit))
        assert all(np.isfinite(v) for v in (noisy, den, nl, reg, reg_d, unfit))
    return rows


def test_cornell_box_is_closer_to_the_oracle_than_the_render_it_was_made_from(scenes):
    """cornell_box 800x800, halves of 8 samples, defaults (mask 7, demodulation, the default ridge), against the oracle's windows at spp 1000
    (tests/golden/golden_windows.npz): in every window the fitted image is closer to the converged one than the mean of the halves."""
    rows = _window_errors(scenes, "cornell_box")
    assert [r[0] for r in rows] == ["t2_cornell_0", "t2_cornell_1", "t2_cornell_2"]
    for key, noisy, _, _, _, reg_d, _ in rows:
        assert reg_d < noisy, (key, noisy, reg_d)


def test_final_scene_table_is_finite(scenes):
    """final_scene 800x800, the same settings: the four windows are printed and only have to be finite (DESIGN.md section 10b has the table;
    t2_final_2, the noise sphere, and t2_final_3, the sphere cluster, are the windows the filter is for)."""
    rows = _window_errors(scenes, "final_scene")
    assert [r[0] for r in rows] == ["t2_final_0", "t2_final_1", "t2_final_2", "t2_final_3"]


def test_cli_writes_the_python_composition(scenes, tmp_path):
    out, fit = tmp_path / "image.png", tmp_path / "fit.png"
    r = subprocess.run([sys.executable, "-m", "rttnw_amd", "7", "--width", "64", "--spp", "16", "--denoise-regress", "--fit-map", str(fit), "--out", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)   # a fresh child process
    assert r.returncode == 0, r.stderr
    assert "first-order regression" in r.stdout
    from PIL import Image
    im = Image.open(out)
    im.load()
    assert im.size == (64, 64) and im.mode == "RGBA"
    a, b, f = _frame(scenes, "cornell_box", 64)
    want = render.denoise_regress(a, b, None, None, f)
    assert np.array_equal(np.asarray(im), want["rgba8"])
    assert np.array_equal(np.asarray(Image.open(fit)), (want["fit"] * 127.5).astype(np.uint8))
