"""rttnw_render_adaptive_denoised on the MI355X, held to its contract (include/rttnw_hip.h): its seven outputs are, bit for bit, those of the host
composition the header states — per round rttnw_render_adaptive_region over the mask of active pixels under a tolerance of 0 and a cap of
(k+1)B, rttnw_denoise on that call's image and squared standard error with the features of rttnw_render_features, and the stopping rule in
numpy — for every precision and launch split.  The composition is built HERE, from entry points that existed before this one and are held to
the oracle by their own tests; the entry point under test never feeds it.  With 0 iterations the filter is the identity and the call is
anchored to rttnw_render_adaptive itself.

Tolerances of the mixed-map cases: TOL below, the issue's starting values; test_equals_the_composition_bit_for_bit's docstring holds the
histograms of n_q the COMPOSITION gives under them."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_cases import build_scenes
from gpu_cases import hist as _histogram
from rttnw_amd import abi, render
from rttnw_amd import scene as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = [abi.F64, abi.F32, abi.F64_STRICT]
W, H, B, CAP, ITERATIONS = 48, 40, 16, 64, 5     # 48x40: 6 x 5 tiles — the frame is no multiple of the 32x8 launch blocks, and 40 = 5 tile rows
TOL = dict(rel=0.05, ab=0.01)                    # the issue's starting values
IMAGES = ("linear", "rgba8", "spp", "stderr", "raw_linear", "raw_stderr")


@pytest.fixture(scope="module")
def scenes(gpu):
    return build_scenes(gpu, ("cornell_box", "simple_light", "final_scene"))


def _setup(scenes, name, precision, w=W, h=H, cap=CAP, spp_chunk=1):
    sc, setup = scenes[name]
    cam, p = S.params_for(setup, w, h, cap, precision=precision, spp_chunk=spp_chunk)
    return sc, cam, p


def compose(sc, cam, p, pass_spp, rel, ab, iterations, feature_spp=0):
    """The header's normative composition, on the host: entry points that existed before rttnw_render_adaptive_denoised, and numpy."""
    h, w, cap = p.height, p.width, p.spp
    pf = copy.copy(p)
    pf.spp = feature_spp or pass_spp
    features = render.render_features(sc, cam, pf)
    active = np.ones((h, w), dtype=bool)
    state, out, rounds = None, None, 0
    for k in range(cap // pass_spp):
        if not active.any():
            break
        pk = copy.copy(p)
        pk.spp = (k + 1) * pass_spp
        lin, _, spp, se, _, state = render.render_adaptive_region(sc, cam, pk, 0, 0, w, h, mask=active, state=state, device_ids=None,
                                                                  pass_spp=pass_spp, rel_error=0.0, abs_error=0.0)
        den, den_rgba, var_f = render.denoise(lin, features, se, iterations=iterations)
        with np.errstate(invalid="ignore"):
            stderr_f = np.sqrt(var_f)
            filtered = (np.isfinite(var_f) & (stderr_f <= ab + rel * den)).all(axis=2)
        own_zero = (se == 0.0).all(axis=2)
        active = active & ~(own_zero | filtered)
        rounds += 1
        out = dict(linear=den, rgba8=den_rgba, spp=spp, stderr=stderr_f, raw_linear=lin, raw_stderr=se, state=state)
    out["rounds"] = rounds
    out["features"] = features
    return out


def _same(got, ref, what=""):
    for key in IMAGES:
        assert np.array_equal(got[key], ref[key], equal_nan=key in ("stderr", "raw_stderr")), (what, key, int((got[key] != ref[key]).sum()))
    assert np.array_equal(got["state"], ref["state"]), (what, "state")


@pytest.fixture(scope="module")
def guided(scenes):
    """The entry point under test per (scene, spp_chunk, precision) on the 48x40 frame under TOL, default launch split: computed once, shared."""
    cache = {}

    def get(name, spp_chunk, precision):
        key = (name, spp_chunk, precision)
        if key not in cache:
            assert "RTTNW_CHUNK_SUM_BUDGET" not in os.environ
            sc, cam, p = _setup(scenes, name, precision, spp_chunk=spp_chunk)
            cache[key] = render.render_adaptive_denoised(sc, cam, p, B, TOL["rel"], TOL["ab"], iterations=ITERATIONS)
            for a in cache[key].values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        return cache[key]
    return get


@pytest.mark.parametrize("precision", PRECISIONS, ids=["f64", "f32", "f64strict"])
@pytest.mark.parametrize("spp_chunk", [1, 0])
@pytest.mark.parametrize("name", ["cornell_box", "final_scene"])
def test_equals_the_composition_bit_for_bit(scenes, guided, name, spp_chunk, precision):
    """48x40, B 16, cap 64, 5 iterations, default sigmas: all six images and state_out equal the composition's.  Not vacuously: the composition ran
    at least two rounds, its samples map holds at least two values, and a pixel stopped before the cap.
    Chosen tolerances: rel_error 0.05, abs_error 0.01 — the values the work started from; the first run on an MI355X gave mixed maps, so nothing
    was changed.  The composition's histogram of n_q (pixels per sample count; 4 rounds in every case; spp_chunk 1 and 0 alike — the Python
    drivers take 0 as max(1, B / 16) = 1):
      cornell_box  f64 and f64strict  {16: 1746, 32: 69, 48: 21, 64: 84}      f32  {16: 1746, 32: 70, 48: 21, 64: 83}
      final_scene  f64 and f64strict  {16: 1504, 32: 29, 48: 28, 64: 359}     f32  {16: 1503, 32: 28, 48: 28, 64: 361}
    (Of cornell_box's 1920 pixels 1244 have a standard error of 0 after round 0 — they see black — and stop on the rule's first condition;
    the other ~500 that stop at 16 do so on the filtered error.)"""
    sc, cam, p = _setup(scenes, name, precision, spp_chunk=spp_chunk)
    ref = compose(sc, cam, p, B, TOL["rel"], TOL["ab"], ITERATIONS)
    print("%s spp_chunk %d precision %d: composition ran %d rounds, n_q histogram %s" % (name, spp_chunk, precision, ref["rounds"], _histogram(ref["spp"])))
    assert ref["rounds"] >= 2
    assert len(np.unique(ref["spp"])) >= 2
    assert (ref["spp"] < CAP).any()
    got = guided(name, spp_chunk, precision)
    _same(got, ref, name)
    assert got["rounds"] == ref["rounds"]
    assert got["stats"].samples == int(ref["spp"].sum(dtype=np.uint64)) and got["stats"].kernel_ms > 0.0


@pytest.mark.parametrize("precision", PRECISIONS, ids=["f64", "f32", "f64strict"])
def test_zero_iterations_is_the_plain_adaptive_render(scenes, precision):
    """iterations = 0: the filter is the identity, so the loop is rttnw_render_adaptive's under the same cap, B and tolerances — samples map, raw and
    'filtered' image, RGBA8, raw standard errors, bit for bit (sqrt(x * x) == x for finite normal doubles; +inf squares and roots to +inf)."""
    sc, cam, p = _setup(scenes, "cornell_box", precision)
    got = render.render_adaptive_denoised(sc, cam, p, B, TOL["rel"], TOL["ab"], iterations=0)
    lin, rgba, spp, se, st = render.render_adaptive(sc, cam, p, B, TOL["rel"], TOL["ab"])
    assert len(np.unique(spp)) >= 2, "the anchor must be a mixed map"
    bad = np.argwhere(got["spp"] != spp)
    assert bad.size == 0, ("samples differ at (row, col)", bad[:8].tolist(), got["spp"][tuple(bad[0])], spp[tuple(bad[0])])
    for key, ref in (("raw_linear", lin), ("linear", lin), ("raw_stderr", se), ("stderr", se)):
        bad = np.argwhere(~((got[key] == ref) | (np.isnan(got[key]) & np.isnan(ref))).all(axis=2))
        assert bad.size == 0, (key, "differs at (row, col)", bad[:8].tolist())
    bad = np.argwhere((got["rgba8"] != rgba).any(axis=2))
    assert bad.size == 0, ("rgba8 differs at (row, col)", bad[:8].tolist(), [got["rgba8"][tuple(q)].tolist() for q in bad[:4]],
                           [rgba[tuple(q)].tolist() for q in bad[:4]], [lin[tuple(q)].tolist() for q in bad[:4]])
    assert got["stats"].samples == st.samples


@pytest.mark.parametrize("precision", PRECISIONS, ids=["f64", "f32", "f64strict"])
def test_the_launch_split_changes_nothing(scenes, guided, monkeypatch, precision):
    """RTTNW_CHUNK_SUM_BUDGET=1: one chunk per launch, sixteen launches per round instead of one — the same seven outputs."""
    ref = guided("cornell_box", 1, precision)
    monkeypatch.setenv("RTTNW_CHUNK_SUM_BUDGET", "1")
    sc, cam, p = _setup(scenes, "cornell_box", precision)
    got = render.render_adaptive_denoised(sc, cam, p, B, TOL["rel"], TOL["ab"], iterations=ITERATIONS)
    _same(got, ref, "split")


@pytest.mark.parametrize("precision", PRECISIONS, ids=["f64", "f32", "f64strict"])
def test_state_out_is_an_ordinary_state(scenes, guided, precision):
    """rttnw_render_adaptive_resume takes state_out under the same cap and a tolerance of 0 and traces what is missing to the cap: cap * w * h -
    sum(out_spp) samples — less those of the pixels whose standard error is 0 in every channel, which a tolerance of 0 leaves alone (counted)."""
    g = guided("cornell_box", 1, precision)
    sc, cam, p = _setup(scenes, "cornell_box", precision)
    lin, rgba, spp, se, st, state = render.render_adaptive_resume(sc, cam, p, g["state"], None, pass_spp=B, rel_error=0.0, abs_error=0.0)
    missing = CAP - g["spp"].astype(np.int64)
    zero = (g["raw_stderr"] == 0.0).all(axis=2)
    print("precision %d: %d samples missing to the cap, %d of them in %d zero-stderr pixels" % (precision, missing.sum(), missing[zero].sum(), zero.sum()))
    assert missing.sum() > 0
    assert st.samples == int(missing[~zero].sum())
    assert st.samples == CAP * W * H - int(g["spp"].sum()) - int(missing[zero].sum())
    assert (spp[~zero] == CAP).all() and np.array_equal(spp[zero], g["spp"][zero])
    # ... and what the resumed render continues is the render the state came from: a pixel already at the cap keeps its bits
    at_cap = g["spp"] == CAP
    assert np.array_equal(lin[at_cap], g["raw_linear"][at_cap]) and np.array_equal(se[at_cap], g["raw_stderr"][at_cap])


def test_cap_equal_to_pass_spp_is_one_round(scenes):
    sc, cam, p = _setup(scenes, "cornell_box", abi.F64, cap=B)
    got = render.render_adaptive_denoised(sc, cam, p, B, TOL["rel"], TOL["ab"], iterations=ITERATIONS)
    ref = compose(sc, cam, p, B, TOL["rel"], TOL["ab"], ITERATIONS)
    assert ref["rounds"] == 1 and got["rounds"] == 1 and (got["spp"] == B).all() and got["stats"].samples == B * W * H
    _same(got, ref, "cap == B")


def test_feature_spp_of_its_own(scenes):
    """feature_spp = 4, not B = 16: other features, another filter, other stopping decisions — and still the composition's."""
    sc, cam, p = _setup(scenes, "cornell_box", abi.F64)
    got = render.render_adaptive_denoised(sc, cam, p, B, TOL["rel"], TOL["ab"], iterations=ITERATIONS, feature_spp=4)
    ref = compose(sc, cam, p, B, TOL["rel"], TOL["ab"], ITERATIONS, feature_spp=4)
    _same(got, ref, "feature_spp 4")
    same_features = compose(sc, cam, p, B, TOL["rel"], TOL["ab"], ITERATIONS)
    assert not np.array_equal(ref["features"]["normal"], same_features["features"]["normal"]), "4 and 16 samples give other silhouettes"
    assert not np.array_equal(got["linear"], same_features["linear"])


@pytest.mark.parametrize("precision", PRECISIONS, ids=["f64", "f32", "f64strict"])
def test_background_pixels_pass_through_and_stop(scenes, precision):
    """simple_light: part of the frame sees the (black) background only.  Such a pixel has alpha 0, so the filter passes it through; every sample
    of it is the background colour, so its own standard error is 0 and it stops after round 0 — the first stopping condition."""
    sc, cam, p = _setup(scenes, "simple_light", precision)
    got = render.render_adaptive_denoised(sc, cam, p, B, TOL["rel"], TOL["ab"], iterations=ITERATIONS)
    ref = compose(sc, cam, p, B, TOL["rel"], TOL["ab"], ITERATIONS)
    _same(got, ref, "simple_light")
    empty = ref["features"]["alpha"] == 0.0
    print("simple_light precision %d: %d of %d pixels are background; n_q histogram %s" % (precision, empty.sum(), empty.size, _histogram(got["spp"])))
    assert empty.any() and not empty.all()
    assert np.array_equal(got["linear"][empty], got["raw_linear"][empty]) and np.array_equal(got["stderr"][empty], got["raw_stderr"][empty])
    assert (got["raw_stderr"][empty] == 0.0).all() and (got["spp"][empty] == B).all()
    assert (got["spp"] % B == 0).all() and got["spp"].min() >= B and got["spp"].max() <= CAP


def test_cli_guided(gpu, tmp_path):
    """python -m rttnw_amd 7 --noise 0.05 --guided in a fresh process: both PNGs, the samples traced and the rounds run."""
    from PIL import Image
    r = subprocess.run([sys.executable, "-m", "rttnw_amd", "7", "--width", "96", "--spp", "64", "--pass-spp", "16", "--noise", "0.05", "--guided",
                        "--spp-map", "m.png"], cwd=tmp_path, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))
    assert r.returncode == 0, r.stderr
    assert Image.open(tmp_path / "image.png").size == (96, 96) and Image.open(tmp_path / "m.png").size == (96, 96)
    assert "samples traced of" in r.stdout and "rounds of 4" in r.stdout and "5 denoise iterations" in r.stdout, r.stdout


def test_the_filtered_image_is_closer_to_the_cap_render_than_the_raw_one(scenes):
    """cornell_box 128x128, B 16, cap 64, TOL: against rttnw_render of the same frame at the cap's spp, the denoised output's MSE is below the raw
    output's — the '> 1 gain' DESIGN.md section 10b asserts of the denoiser, here of the image this entry point leaves.  Measured: raw 0.0361,
    denoised 0.0236 (ratio 1.53) at 266 704 of 1 048 576 samples; n_q histogram {16: 16229, 32: 78, 48: 24, 64: 53}."""
    sc, cam, p = _setup(scenes, "cornell_box", abi.F64, w=128, h=128)
    got = render.render_adaptive_denoised(sc, cam, p, B, TOL["rel"], TOL["ab"], iterations=ITERATIONS)
    full, _, _ = render.render_host(sc, cam, p)
    mse_raw, mse_den = float(((got["raw_linear"] - full) ** 2).mean()), float(((got["linear"] - full) ** 2).mean())
    print("MSE against the %d-spp render: raw %.4g, denoised %.4g, ratio %.2f; %d samples of %d; n_q histogram %s"
          % (CAP, mse_raw, mse_den, mse_raw / mse_den, got["stats"].samples, CAP * 128 * 128, _histogram(got["spp"])))
    assert mse_den < mse_raw

