"""rttnw_render_preview on the MI355X, held to its contract (include/rttnw_hip.h): every output is, bit for bit, that of the host composition the
header states — rttnw_render_adaptive_region over the mask of the lattice, rttnw_render_features, rttnw_reconstruct without a variance — for every
precision and launch split; the composition is built HERE from those entry points, the one under test never feeds it.  Level 0 is anchored to
rttnw_render_adaptive and rttnw_denoise, the state to rttnw_render_adaptive_resume's, and the picture to the CPU oracle's converged windows."""
import copy
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from golden_cases import WINDOWS, load_windows
from gpu_cases import build_scenes
from rttnw_amd import abi, render
from rttnw_amd import scene as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = [abi.F64, abi.F64_STRICT, abi.F32]
SIZES = [(96, 96), (45, 37)]           # 45x37: ragged against the 8x8 tiles, the 2x2 blocks and every lattice; its level-6 lattice is one pixel
LEVELS = (0, 2, 6)
B, CAP, REL = 16, 32, 0.1
IMAGES = ("linear", "rgba8", "valid", "spp", "raw_linear", "raw_stderr")


@pytest.fixture(scope="module")
def scenes(gpu):
    return build_scenes(gpu, ("cornell_box", "final_scene"))


def _setup(scenes, name, precision, size, cap=CAP):
    sc, setup = scenes[name]
    cam, p = S.params_for(setup, size[0], size[1], cap, precision=precision)
    return sc, cam, p


def compose(sc, cam, p, level, pass_spp, rel, iterations=5, feature_spp=0):
    """The header's normative composition, on the host: entry points that existed before rttnw_render_preview, and rttnw_reconstruct."""
    h, w = p.height, p.width
    lin, _, spp, se, st, state = render.render_adaptive_region(sc, cam, p, 0, 0, w, h, mask=render.lattice_mask(w, h, level), state=None,
                                                               device_ids=None, pass_spp=pass_spp, rel_error=rel, abs_error=0.0)
    pf = copy.copy(p)
    pf.spp = feature_spp or pass_spp
    features = render.render_features(sc, cam, pf)
    out, rgba, _, ok = render.reconstruct(lin, spp > 0, features, None, iterations=iterations)
    return dict(linear=out, rgba8=rgba, valid=ok, spp=spp, raw_linear=lin, raw_stderr=se, state=state, samples=st.samples)


def _same(got, ref, what=""):
    for key in IMAGES:
        assert np.array_equal(got[key], ref[key], equal_nan=key == "raw_stderr"), (what, key, int((got[key] != ref[key]).sum()))
    assert np.array_equal(got["state"], ref["state"]), (what, "state")


@pytest.mark.parametrize("precision", PRECISIONS, ids=["f64", "f64strict", "f32"])
@pytest.mark.parametrize("size", SIZES, ids=["96x96", "45x37"])
@pytest.mark.parametrize("name", ["cornell_box", "final_scene"])
def test_equals_the_composition_bit_for_bit(scenes, name, size, precision):
    """B 16, cap 32, rel_error 0.1, 5 iterations, default sigmas, levels 0, 2 and 6: all six images and state_out equal the composition's, the
    samples reported are the samples map's sum, and no pixel off the lattice was traced.  Not vacuously: on cornell_box the lattice holds pixels
    that stopped after one pass (those that see black) and pixels that went to the cap."""
    sc, cam, p = _setup(scenes, name, precision, size)
    for level in LEVELS:
        ref = compose(sc, cam, p, level, B, REL)
        got = render.render_preview(sc, cam, p, level, pass_spp=B, rel_error=REL)
        _same(got, ref, level)
        on = render.lattice_mask(size[0], size[1], level) != 0
        assert (got["spp"][~on] == 0).all() and (got["spp"][on] >= B).all() and (got["spp"][on] % B == 0).all()
        assert got["stats"].samples == int(got["spp"].sum()) == ref["samples"]
        assert (got["raw_linear"][~on] == 0.0).all() and (got["raw_stderr"][~on] == 0.0).all()
        records = got["state"][64:].reshape(size[1], size[0], 12)
        assert (records[~on] == 0.0).all() and (records[on][:, 3] == got["spp"][on]).all()
        assert (got["valid"][on] == 1).all()
        if name == "cornell_box" and level in (0, 2) and size == (96, 96):
            assert set(np.unique(got["spp"][on])) == {B, CAP}, np.unique(got["spp"][on])
    # a feature_spp and a filter of the caller's travel to the device
    ref = compose(sc, cam, p, 2, B, REL, iterations=2, feature_spp=4)
    got = render.render_preview(sc, cam, p, 2, pass_spp=B, rel_error=REL, iterations=2, feature_spp=4)
    _same(got, ref, "feature_spp 4, 2 iterations")


@pytest.mark.parametrize("precision", PRECISIONS, ids=["f64", "f64strict", "f32"])
def test_the_launch_split_changes_nothing(scenes, monkeypatch, precision):
    """RTTNW_CHUNK_SUM_BUDGET=1: one chunk per launch, sixteen launches per round instead of one — the same outputs."""
    sc, cam, p = _setup(scenes, "cornell_box", precision, (45, 37))
    ref = render.render_preview(sc, cam, p, 2, pass_spp=B, rel_error=REL)
    monkeypatch.setenv("RTTNW_CHUNK_SUM_BUDGET", "1")
    got = render.render_preview(sc, cam, p, 2, pass_spp=B, rel_error=REL)
    _same(got, ref, "split")
    _same(got, compose(sc, cam, p, 2, B, REL), "split against the composition under the same split")


@pytest.mark.parametrize("precision", PRECISIONS, ids=["f64", "f64strict", "f32"])
def test_level_0_is_the_adaptive_render_denoised(scenes, precision):
    sc, cam, p = _setup(scenes, "cornell_box", precision, (45, 37))
    got = render.render_preview(sc, cam, p, 0, pass_spp=B, rel_error=REL)
    lin, rgba, spp, se, st = render.render_adaptive(sc, cam, p, pass_spp=B, rel_error=REL)
    assert np.array_equal(got["raw_linear"], lin) and np.array_equal(got["spp"], spp) and np.array_equal(got["raw_stderr"], se, equal_nan=True)
    pf = copy.copy(p)
    pf.spp = B
    den, den_rgba, _ = render.denoise(lin, render.render_features(sc, cam, pf), None)
    assert np.array_equal(got["linear"], den) and np.array_equal(got["rgba8"], den_rgba) and (got["valid"] == 1).all()
    assert got["stats"].samples == st.samples


@pytest.mark.parametrize("precision", PRECISIONS, ids=["f64", "f64strict", "f32"])
def test_state_out_completes_to_the_fresh_adaptive_render(scenes, precision):
    """rttnw_render_adaptive_region over the whole frame takes state_out and traces only what the lattice left out; what it leaves is the state of
    the adaptive render that never was a preview, bit for bit."""
    size = (45, 37)
    sc, cam, p = _setup(scenes, "cornell_box", precision, size)
    got = render.render_preview(sc, cam, p, 2, pass_spp=B, rel_error=REL)
    lin, _, spp, se, st, state = render.render_adaptive_region(sc, cam, p, 0, 0, size[0], size[1], state=got["state"], pass_spp=B, rel_error=REL)
    f_lin, _, f_spp, f_se, f_st, f_state = render.render_adaptive_resume(sc, cam, p, None, None, pass_spp=B, rel_error=REL)
    assert np.array_equal(state, f_state)
    assert np.array_equal(lin, f_lin) and np.array_equal(spp, f_spp) and np.array_equal(se, f_se, equal_nan=True)
    assert st.samples == int(spp.sum()) - int(got["spp"].sum()) and st.samples > 0      # ... and no lattice pixel was traced again


def test_cli_preview_then_the_rest_of_the_frame(scenes, tmp_path):
    """python -m rttnw_amd 7 --noise 0.1 --preview 2 --save-state in a fresh process, then --resume --refine over the frame in another: the image,
    the samples map and the state are written, every pixel holds a value, and the two runs together trace what one adaptive render traces."""
    from PIL import Image
    base = [sys.executable, "-m", "rttnw_amd", "7", "--width", "96", "--spp", "32", "--pass-spp", "16", "--noise", "0.1"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    traced = []
    for extra in (["--preview", "2", "--spp-map", "m.png", "--save-state", "lattice.npy"], ["--resume", "lattice.npy", "--refine", "0,0,96,96"]):
        r = subprocess.run(base + extra, cwd=tmp_path, capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stderr
        assert Image.open(tmp_path / "image.png").size == (96, 96)
        traced.append(int(re.search(r"adaptive: (\d+) samples traced", r.stdout).group(1)))
        if "--preview" in extra:
            assert "preview: 1 pixel in 16, 9216 of 9216 pixels hold a value, 5 denoise iterations" in r.stdout, r.stdout
            assert Image.open(tmp_path / "m.png").size == (96, 96)
            assert np.array(Image.open(tmp_path / "image.png"))[..., 3].min() == 255
            state = np.load(tmp_path / "lattice.npy")[64:].reshape(96, 96, 12)
            on = render.lattice_mask(96, 96, 2) != 0
            assert (state[~on] == 0.0).all() and (state[on][:, 3] >= 16).all()
    sc, cam, p = _setup(scenes, "cornell_box", abi.F64, (96, 96))
    assert traced[0] + traced[1] == render.render_adaptive(sc, cam, p, pass_spp=B, rel_error=REL)[4].samples and 0 < traced[0] < traced[1]


def _nearest_fill(raw, level):
    """Every pixel takes the value of the nearest lattice pixel (a tie goes to the one further right / down; the last lattice row and column
    serve what lies beyond them)."""
    h, w = raw.shape[:2]
    step = 1 << level
    ys = np.minimum((np.arange(h) + step // 2) // step * step, (h - 1) // step * step)
    xs = np.minimum((np.arange(w) + step // 2) // step * step, (w - 1) // step * step)
    return raw[ys][:, xs]


def _window_errors(scenes, name, level=2, spp=16):
    """Per committed oracle window of the 800x800 frame: (key, MSE of the preview, of the nearest-lattice fill of the same raw values, of the plain
    render at the same spp, share of the window's pixels that hold a value)."""
    sc, cam, p = _setup(scenes, name, abi.F64, (800, 800), cap=spp)
    got = render.render_preview(sc, cam, p, level, pass_spp=spp, rel_error=0.0)
    on = render.lattice_mask(800, 800, level) != 0
    assert (got["spp"][on] == spp).all() and (got["spp"][~on] == 0).all()
    fill = _nearest_fill(got["raw_linear"], level)
    plain, _, _ = render.render_host(sc, cam, p)
    gold = load_windows()
    rows = []
    for key, scene, w, h, _, x0, y0, cw, ch, _ in WINDOWS:
        if scene != name or not key.startswith("t2_"):
            continue
        ref = gold[key + "_linear"]
        crop = (slice(y0, y0 + ch), slice(x0, x0 + cw))
        mse = lambda img: float(np.mean((img[crop] - ref) ** 2))
        rows.append((key, mse(got["linear"]), mse(fill), mse(plain), float(got["valid"][crop].mean())))
    return rows, got["stats"].kernel_ms


def _print(rows, ms):
    for key, pre, fill, plain, share in rows:
        print("%s level 2: MSE preview %.4g, nearest fill %.4g (x%.1f), plain 16 spp %.4g (x%.1f), valid %.4f"
              % (key, pre, fill, fill / pre, plain, plain / pre, share))
    print("kernel_ms %.2f" % ms)


def test_a_preview_is_closer_to_the_converged_frame_than_its_samples_or_the_full_noisy_render(scenes):
    """cornell_box 800x800, B = cap = 16, a tolerance of 0, level 2 (1/16 of the pixels), default parameters, against the oracle's windows at spp
    1000 (tests/golden/golden_windows.npz): in every window every pixel holds a value, and the reconstruction is closer to the converged image
    than the nearest-lattice fill of the same raw values AND than the plain 16-spp render of every pixel.  (A numpy prototype on the CPU oracle's
    frames gave margins of about 40x and 25x.)  Measured on an MI355X, MSE preview / nearest fill / plain 16 spp: 0.001052 / 0.04105 / 0.02871,
    0.000708 / 0.03015 / 0.02782, 0.001131 / 0.04813 / 0.04421 in t2_cornell_0..2."""
    rows, ms = _window_errors(scenes, "cornell_box")
    assert [r[0] for r in rows] == ["t2_cornell_0", "t2_cornell_1", "t2_cornell_2"]
    _print(rows, ms)
    for key, pre, fill, plain, share in rows:
        assert share == 1.0, key
        assert pre < fill, (key, pre, fill)
        assert pre < plain, (key, pre, plain)


def test_final_scene_windows_are_recorded(scenes):
    """final_scene's four windows — earth and the blue medium, the glass sphere, the noise sphere, the sphere cluster: where a filter guided by the
    FIRST hit is weakest, and where a lattice misses what is smaller than its spacing.  Recorded, not asserted (DESIGN.md section 10b,
    profiles/LEDGER.md); the run only has to be finite.  Measured, MSE preview / nearest fill / plain 16 spp: 0.000859 / 0.01601 / 0.01621,
    0.000213 / 0.004364 / 0.00479, 0.0111 / 0.06288 / 0.04563, 0.005557 / 0.01018 / 0.009057 in t2_final_0..3."""
    rows, ms = _window_errors(scenes, "final_scene")
    assert len(rows) == 4
    _print(rows, ms)
    for key, pre, fill, plain, share in rows:
        assert np.isfinite(pre) and np.isfinite(fill) and np.isfinite(plain)
