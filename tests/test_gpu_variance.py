"""rttnw_temporal_variance on the MI355X: the device kernels equal the numpy restatement of the header bit for bit along chains of three calls
on frames that cross the kernels' blocks, and the host build of the same header (tests/variance_host) on real renders; stage A is
rttnw_temporal_accumulate; the properties of tests/variance_cases.py hold; the estimate agrees with the adaptive render's own standard error
within a factor of two; what the variance buys rttnw_denoise along an orbit is printed against the CPU oracle's converged windows."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

import variance_ref
from golden_cases import WINDOWS, load_windows
from temporal_cases import same
from variance_cases import (CASE_IDS, CASES, assert_same_outputs, check_chain, check_constant_input, check_miss_pixels, check_spatial_branch_is_unbiased,
                            check_temporal_branch_is_unbiased, check_window_respects_edges)
from rttnw_amd import abi, library, render
from rttnw_amd import scene as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
device = render.temporal_variance


@pytest.fixture(scope="module")
def host():
    return variance_ref.host()


@pytest.fixture(scope="module")
def scenes(gpu):
    lib = library.scenes()
    return {name: S.build(gpu, lib, name, S.load_earth() if name == "final_scene" else None) for name in ("cornell_box", "final_scene")}


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_device_equals_the_numpy_restatement_bit_for_bit(gpu, case):
    """The cases of tests/test_variance_cpu.py — 70x41 crosses the 64-wide blocks and is no multiple of 4 rows, the halo meets every border of the
    image at 3x5 —, and stage A against rttnw_temporal_accumulate itself."""
    check_chain(device, variance_ref.estimate, render.temporal_accumulate, case)


@pytest.mark.parametrize("name", ["cornell_box", "final_scene"])
def test_device_equals_host_harness_on_real_frames(scenes, host, name):
    """96x96, 8 samples a frame, three cameras 2 degrees apart on the orbit: the first call without a history, then a chain over the results."""
    sc, setup = scenes[name]
    cam, p = S.params_for(setup, 96, 96, 8, precision=abi.F64)
    history = None
    for k, c in enumerate(render.orbit_cameras(cam, 3, 2.0)):
        pk = copy.copy(p)
        pk.sample_begin = k * p.spp
        lin, f = render.render_host(sc, c, pk)[0], render.render_features(sc, c, pk)
        got = device(lin, f, c, history=history, min_temporal=2 + k % 2)
        assert_same_outputs(got, host(lin, f, c, history=history, min_temporal=2 + k % 2), (k,))
        plain = render.temporal_accumulate(lin, f, c, history=None if history is None else dict(history, variance=None))
        for key in ("linear", "rgba8", "length", "prev_xy"):
            assert same(got[key], plain[key]), (key, k)
        history = got
    hit = f["alpha"] != 0.0
    assert np.isfinite(got["variance"]).all() and (got["variance"][hit] > 0.0).any()
    assert (got["length"][hit] >= 2.0).mean() > 0.5 and (got["length"][hit] == 1.0).any()          # both branches


def test_constant_input_has_no_variance(gpu):
    check_constant_input(device)


def test_both_branches_are_unbiased(gpu):
    print("temporal branch, variance * 8 over sigma^2 (left, right):", check_temporal_branch_is_unbiased(device))
    print("spatial branch, variance over sigma^2 (left, right):", check_spatial_branch_is_unbiased(device))


def test_the_window_respects_edges_and_misses(gpu):
    check_window_respects_edges(device)
    check_miss_pixels(device)


def test_the_estimate_agrees_with_the_adaptive_renders_standard_error(scenes):
    """cornell_box 96x96, a static camera, 8 frames of 4 samples at sample_begin 0, 4, ..., 28, features at 32 samples: every pixel that hit is
    on the temporal branch after the last frame.  The sum of its variances against the sum of stderr^2 of rttnw_render_adaptive over the same
    32 samples (one pass of 32, cap 32): two estimates of one quantity from the same samples — the one from eight group means of four is the
    noisier.  The ratio of sums lies in [0.5, 2]: a gross condition that catches a missing division by N or a wrong group factor (4 or more),
    not a precision claim.  Measured: 708.07 against 714.99, ratio 0.990 over 8464 pixels."""
    sc, setup = scenes["cornell_box"]
    cam, p = S.params_for(setup, 96, 96, 4, precision=abi.F64)
    _, p32 = S.params_for(setup, 96, 96, 32, precision=abi.F64)
    f = render.render_features(sc, cam, p32)
    history = None
    for k in range(8):
        pk = copy.copy(p)
        pk.sample_begin = 4 * k
        history = device(render.render_host(sc, cam, pk)[0], f, cam, history=history, max_history=32)
    hit = f["alpha"] != 0.0
    assert hit.mean() > 0.5 and np.all(history["length"][hit] == 8.0)
    _, _, n, se, _ = render.render_adaptive(sc, cam, p32, pass_spp=32, rel_error=0.0)
    assert (n == 32).all()
    ours, theirs = float(history["variance"][hit].sum()), float(np.square(se)[hit].sum())
    print("calibration: sum of out_variance_rgb %.6g, sum of stderr^2 %.6g, ratio %.4f over %d pixels" % (ours, theirs, ours / theirs, hit.sum()))
    assert 0.5 <= ours / theirs <= 2.0


@pytest.mark.parametrize("name", ["cornell_box", "final_scene"])
def test_what_the_variance_buys_the_filter_along_an_orbit_is_reported(scenes, name):
    """Printed, not asserted — the finding of DESIGN.md section 10b: the orbit of tests/test_gpu_temporal.py (800x800, 8 frames of 4 samples, 1
    degree a frame), MSE against the oracle's t2_* windows of rttnw_denoise of the accumulated frame without a variance, with out_variance_rgb,
    and of the single frame."""
    sc, setup = scenes[name]
    cam, p = S.params_for(setup, 800, 800, 4, precision=abi.F64)
    last = render.render_sequence(sc, render.orbit_cameras(cam, 8, 1.0), p, variance=True)[-1]
    acc = last["accumulated"]
    images = {"without": render.denoise(acc["linear"], last["features"])[0],
              "with": render.denoise(acc["linear"], last["features"], variance=acc["variance"])[0],
              "single": render.denoise(last["raw"], last["features"])[0]}
    gold = load_windows()
    hit = last["features"]["alpha"] != 0.0
    print("%s: %.1f %% of the pixels that hit took the spatial estimate" % (name, 100.0 * (acc["length"][hit] < 4.0).mean()))
    keys = []
    for key, scene, w, h, spp, x0, y0, cw, ch, _ in WINDOWS:
        if scene != name or not key.startswith("t2_"):
            continue
        keys.append(key)
        ref = gold[key + "_linear"]
        crop = (slice(y0, y0 + ch), slice(x0, x0 + cw))
        r = {k: float(np.mean((v[crop] - ref) ** 2)) for k, v in images.items()}
        print("%s: MSE of rttnw_denoise of the accumulated frame without a variance %.4g, with out_variance_rgb %.4g (%.3f of it), of the single "
              "frame %.4g" % (key, r["without"], r["with"], r["with"] / r["without"], r["single"]))
        assert all(np.isfinite(v) for v in r.values())
    assert len(keys) == (3 if name == "cornell_box" else 4)


def test_cli_writes_the_python_composition(scenes, tmp_path):
    out = tmp_path / "image.png"
    r = subprocess.run([sys.executable, "-m", "rttnw_amd", "7", "--width", "64", "--spp", "4", "--orbit", "3", "--temporal-variance", "--denoise", "--out",
                        str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300)   # a fresh child process
    assert r.returncode == 0, r.stderr
    assert "3 frames of 4 spp" in r.stdout and "temporal:" in r.stdout and "temporal-variance:" in r.stdout
    from PIL import Image
    sc, setup = scenes["cornell_box"]
    cam, p = S.params_for(setup, 64, 64, 4, precision=abi.F64)
    want = render.render_sequence(sc, render.orbit_cameras(cam, 3, 1.0), p, denoise=True, variance=True)
    plain = render.render_sequence(sc, render.orbit_cameras(cam, 3, 1.0), p, denoise=True)
    for k in range(3):
        im = Image.open(tmp_path / ("frame_%03d.png" % k))
        im.load()
        assert np.array_equal(np.asarray(im), want[k]["rgba8"]), k
    assert not np.array_equal(want[2]["rgba8"], plain[2]["rgba8"])                         # the variance reached the filter
    assert same(want[2]["accumulated"]["linear"], plain[2]["accumulated"]["linear"])       # ... and left the accumulation alone
