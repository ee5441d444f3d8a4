"""rttnw_denoise_nlm on the MI355X: the device kernels equal the host build of the same header (tests/nlm_host) bit for bit, on synthetic frames
that cross the kernel's tiles and on real half renders; the exchange of the halves and locality hold on the device; the filter lowers the error
against the CPU oracle's converged windows — never against ourselves — and beats the feature-guided filter where first-hit features say
nothing; the command line writes what the Python composition computes."""
import os
import subprocess
import sys

import numpy as np
import pytest

import nlm_ref
from golden_cases import WINDOWS, load_windows
from nlm_cases import FRAMES, KS, RADII, crop_interior, same_bits, swapped_equal
from rttnw_amd import abi, library, render
from rttnw_amd import scene as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host():
    return nlm_ref.host()


@pytest.fixture(scope="module")
def scenes(gpu):
    lib = library.scenes()
    return {name: S.build(gpu, lib, name, S.load_earth() if name == "final_scene" else None) for name in ("cornell_box", "final_scene")}


def _halves(scenes, name, w, spp=16, with_variance=False):
    """(half_a, half_b, var_a, var_b) of a frame: two plain renders of spp / 2 samples over disjoint sample ranges — or, for the variances of the
    halves' pixel means, two adaptive renders that run to their cap of spp / 2 and report their noise (stderr squared)."""
    sc, setup = scenes[name]
    cam, p = S.params_for(setup, w, w, spp, precision=abi.F64)
    if not with_variance:
        (a, _, _), (b, _, _) = render.render_halves(sc, cam, p)
        return a, b, None, None
    out = []
    for k in range(2):
        cam, ph = S.params_for(setup, w, w, spp // 2, precision=abi.F64, sample_begin=k * (spp // 2))
        lin, _, n, se, _ = render.render_adaptive(sc, cam, ph, pass_spp=spp // 2, rel_error=0.0)
        assert (n == spp // 2).all()
        out.append((lin, np.square(se)))
    return out[0][0], out[1][0], out[0][1], out[1][1]


@pytest.fixture(scope="module")
def renders96(scenes):
    """The 96x96 half renders the tests below share, made once: {(scene, with_variance): (a, b, var_a, var_b)}."""
    return {(name, v): _halves(scenes, name, 96, 16, v) for name in ("cornell_box", "final_scene") for v in (False, True)}


def _assert_device_equals_host(host, a, b, va, vb, r=0, f=0, k=0.0):
    got = render.denoise_nlm(a, b, va, vb, search_radius=r, patch_radius=f, k=k)
    want = host(a, b, va, vb, r, f, k)
    for name in nlm_ref.OUTPUTS:
        assert same_bits(got[name], want[name]), (name, r, f, k, va is not None, float(np.nanmax(np.abs(got[name].astype(np.float64) - want[name]))))
    return got


@pytest.mark.parametrize("radii", RADII, ids=lambda rf: "r%d-f%d" % rf)
@pytest.mark.parametrize("size", FRAMES, ids=lambda s: "%dx%d" % s)
def test_device_equals_host_harness_on_frames_that_cross_the_tiles(gpu, host, size, radii):
    """The frames and parameter sets of tests/test_nlm_cpu.py: 33x18 and 37x29 cross the 16-pixel tiles in both axes, 1x1 and 3x5 are all halo."""
    for with_variance in (True, False):
        rng = np.random.default_rng(size[0] * 64 + radii[0] * 2 + int(with_variance))
        a, b, va, vb = nlm_ref.random_inputs(rng, size[0], size[1], with_variance)
        for k in KS:
            _assert_device_equals_host(host, a, b, va, vb, radii[0], radii[1], k)


@pytest.mark.parametrize("with_variance", [True, False], ids=["variance", "pair-variance"])
@pytest.mark.parametrize("name", ["cornell_box", "final_scene"])
def test_device_equals_host_harness_on_real_half_renders(renders96, host, name, with_variance):
    a, b, va, vb = renders96[(name, with_variance)]
    got = _assert_device_equals_host(host, a, b, va, vb)
    assert np.isfinite(got["linear"]).all() and not np.array_equal(got["linear"], (a + b) * 0.5)
    _assert_device_equals_host(host, a, b, va, vb, 10, 3, 0.45)


def _exchange_and_locality(a, b, va, vb, crop):
    """Tests 2 and 3 of tests/test_nlm_cpu.py on the device, at the default radii: swapping the halves, and a crop with a margin of r + f + 1."""
    whole = render.denoise_nlm(a, b, va, vb)
    swapped_equal(whole, render.denoise_nlm(b, a, vb, va))
    m = nlm_ref.DEFAULTS["search_radius"] + nlm_ref.DEFAULTS["patch_radius"] + 1
    part = render.denoise_nlm(a[crop], b[crop], None if va is None else va[crop], None if vb is None else vb[crop])
    assert min(crop_interior(part["linear"], m).shape[:2]) >= 5
    for name in nlm_ref.OUTPUTS:
        assert same_bits(crop_interior(part[name], m), crop_interior(whole[name][crop], m)), name
    short = m - 1 if va is None else m - 2            # (the margin is not generous: tests/test_nlm_cpu.py says why these two)
    assert not same_bits(crop_interior(part["linear"], short), crop_interior(whole["linear"][crop], short))


@pytest.mark.parametrize("with_variance", [True, False], ids=["variance", "pair-variance"])
def test_exchange_and_locality_on_a_synthetic_frame(gpu, with_variance):
    a, b, va, vb = nlm_ref.random_inputs(np.random.default_rng(7), 37, 29, with_variance)
    _exchange_and_locality(a, b, va, vb, (slice(1, 28), slice(4, 33)))            # a 29x27 crop: an interior of 7x5


@pytest.mark.parametrize("with_variance", [True, False], ids=["variance", "pair-variance"])
def test_exchange_and_locality_on_final_scene(renders96, with_variance):
    a, b, va, vb = renders96[("final_scene", with_variance)]
    _exchange_and_locality(a, b, va, vb, (slice(10, 75), slice(21, 90)))          # origin and size off the tile grid


def _window_errors(scenes, name):
    """Per committed oracle window of the 800x800 frame, halves of 8 samples, default parameters: (key, MSE of (a + b) / 2, MSE of rttnw_denoise of
    that mean with the features of 16 samples and no variance, MSE of rttnw_denoise_nlm with the pair variance, the same with given variances)."""
    sc, setup = scenes[name]
    a, b, _, _ = _halves(scenes, name, 800, 16, False)
    mean = (a + b) * 0.5
    nlm = render.denoise_nlm(a, b)["linear"]
    cam, p = S.params_for(setup, 800, 800, 16, precision=abi.F64)
    guided, _, _ = render.denoise(mean, render.render_features(sc, cam, p))
    a2, b2, va, vb = _halves(scenes, name, 800, 16, True)
    nlm_var = render.denoise_nlm(a2, b2, va, vb)["linear"]
    gold = load_windows()
    rows = []
    for key, scene, w, h, spp, x0, y0, cw, ch, _ in WINDOWS:
        if scene != name or not key.startswith("t2_"):
            continue
        ref = gold[key + "_linear"]
        crop = (slice(y0, y0 + ch), slice(x0, x0 + cw))
        rows.append((key,) + tuple(float(np.mean((img[crop] - ref) ** 2)) for img in (mean, guided, nlm, nlm_var)))
    for key, noisy, den, pair, given in rows:
        print("%s: MSE plain 16 spp %.4g, rttnw_denoise %.4g, nlm pair variance %.4g (%.1fx plain, %.2fx rttnw_denoise), nlm given variance %.4g"
              % (key, noisy, den, pair, noisy / pair, den / pair, given))
        assert all(np.isfinite(v) for v in (noisy, den, pair, given))
    return rows


def test_cornell_box_is_closer_to_the_oracle_than_the_render_it_was_made_from(scenes):
    """cornell_box 800x800, halves of 8 samples, pair variance, default parameters, against the oracle's windows at spp 1000
    (tests/golden/golden_windows.npz): in every window the filtered image is closer to the converged one than the mean of the halves.  (numpy
    prototype of the same arithmetic: 32 - 43x.  Measured on the device: 43.3, 31.9, 43.5 with the pair variance; DESIGN.md section 10b has
    the table.)"""
    rows = _window_errors(scenes, "cornell_box")
    assert [r[0] for r in rows] == ["t2_cornell_0", "t2_cornell_1", "t2_cornell_2"]
    for key, noisy, _, pair, _ in rows:
        assert pair < noisy, (key, noisy, pair)


def test_final_scene_beats_the_feature_guided_filter_where_first_hit_features_say_nothing(scenes):
    """final_scene 800x800, the same settings: on the noise sphere (t2_final_2) and the mirror-like sphere cluster (t2_final_3) the filtered image
    is closer to the oracle than rttnw_denoise (defaults, no variance, features of the 16 samples) of the same 16 samples, run here in the same
    process.  (numpy prototype: 2.0x and 5.7x; measured on the device: 2.02x and 5.74x, and 1.12x and 1.24x in t2_final_0 and _1.)  The other
    windows and the given-variance flavour are printed and only have to be finite."""
    rows = {r[0]: r for r in _window_errors(scenes, "final_scene")}
    assert sorted(rows) == ["t2_final_0", "t2_final_1", "t2_final_2", "t2_final_3"]
    for key in ("t2_final_2", "t2_final_3"):
        _, _, den, pair, _ = rows[key]
        assert pair < den, (key, den, pair)


def test_cli_writes_the_python_composition(scenes, tmp_path):
    out = tmp_path / "image.png"
    r = subprocess.run([sys.executable, "-m", "rttnw_amd", "7", "--width", "64", "--spp", "16", "--denoise-nlm", "--out", str(out)], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)   # a fresh child process
    assert r.returncode == 0, r.stderr
    assert "non-local means" in r.stdout
    from PIL import Image
    im = Image.open(out)
    im.load()
    assert im.size == (64, 64) and im.mode == "RGBA"
    a, b, _, _ = _halves(scenes, "cornell_box", 64, 16, False)
    assert np.array_equal(np.asarray(im), render.denoise_nlm(a, b)["rgba8"])
    odd = subprocess.run([sys.executable, "-m", "rttnw_amd", "7", "--width", "64", "--spp", "15", "--denoise-nlm", "--out", str(tmp_path / "odd.png")],
                         cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert odd.returncode == 1 and "even --spp" in odd.stderr and not (tmp_path / "odd.png").exists()
