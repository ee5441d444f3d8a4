"""rttnw_temporal_clamp, rttnw_svgf_set_clamp and rttnw_svgf_clipped on the MI355X: the device kernel equals the numpy restatement of the header bit
for bit along chains of three calls on frames that cross the kernel's blocks and its tile's halo, and the host build of the same header
(tests/clamp_host) on real renders; with gamma = +inf it is rttnw_temporal_variance; the properties of tests/clamp_cases.py hold; a clamped
rttnw_svgf handle equals the composition the header writes down, made with the product's own calls; the command line writes the Python
composition."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

import clamp_ref
import svgf_cases
from clamp_cases import (CASE_IDS, CASES, assert_same_outputs, chain, check_a_ghost_goes, check_chain, check_miss_pixels, check_noise_stays,
                         check_the_window_respects_edges)
from temporal_cases import same
from rttnw_amd import abi, library, render
from rttnw_amd import scene as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
device = render.temporal_clamp
INF = float("inf")


@pytest.fixture(scope="module")
def host():
    return clamp_ref.host()


@pytest.fixture(scope="module")
def scenes(gpu):
    lib = library.scenes()
    return {name: S.build(gpu, lib, name, S.load_earth() if name == "final_scene" else None) for name in ("cornell_box", "final_scene")}


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_device_equals_the_numpy_restatement_bit_for_bit(gpu, case):
    """The cases of tests/test_clamp_cpu.py — 70x41 crosses the 64-wide blocks and the tile's halo and is no multiple of 4 rows, 1x1 and 3x5 are
    smaller than a tile, radius 4 is the largest tile."""
    check_chain(device, case)


def test_a_first_frame_clips_nothing(gpu):
    """No history: every pixel passes through, and the statistics — which the Python driver always asks for, so the blocks with a hit stage their
    tiles for them alone — are the restatement's.  (A first frame of a clamped handle asks for none: no block stages; the handle tests run one.)"""
    for case in (CASES[-1], CASES[4]):
        lin, f, cam = chain(case)[1][0]
        got, want = device(lin, f, cam, clamp_radius=case[1], gamma=case[2]), clamp_ref.clamp(lin, f, cam, clamp_radius=case[1], gamma=case[2])
        assert_same_outputs(got, want)
        assert not got["clipped"].any() and np.all(got["length"] == 1.0)


def test_a_ghost_goes(gpu):
    check_a_ghost_goes(device, render.temporal_variance)


def test_noise_stays(gpu):
    print("share of clipped channels per frame, variance * 8 over sigma^2 (left, right):", check_noise_stays(device))


def test_the_window_respects_edges_and_misses(gpu):
    check_the_window_respects_edges(device)
    check_miss_pixels(device)


def real_frames(sc, setup, count=2):
    cam, p = S.params_for(setup, 96, 96, 8, precision=abi.F64)
    out = []
    for k, c in enumerate(render.orbit_cameras(cam, count, 2.0)):
        pk = copy.copy(p)
        pk.sample_begin = k * p.spp
        out.append((render.render_host(sc, c, pk)[0], render.render_features(sc, c, pk), c))
    return out


def test_gamma_inf_is_temporal_variance_on_the_device(scenes):
    """96x96 cornell_box, two cameras two degrees apart: every shared output, bit for bit, and nothing clipped."""
    sc, setup = scenes["cornell_box"]
    clamped = plain = None
    for k, (lin, f, c) in enumerate(real_frames(sc, setup)):
        clamped = device(lin, f, c, history=clamped, gamma=INF)
        plain = render.temporal_variance(lin, f, c, history=plain)
        assert_same_outputs(clamped, plain, (k,), clamp_ref.SHARED)
        assert not clamped["clipped"].any()
    assert (clamped["length"] == 2.0).mean() > 0.5


@pytest.mark.parametrize("name", ["cornell_box", "final_scene"])
def test_device_equals_host_harness_on_real_frames(scenes, host, name):
    """96x96, 8 samples a frame, two cameras 2 degrees apart, gamma 1: every output; some channels are clipped and some pixels with a history are not."""
    sc, setup = scenes[name]
    history = None
    for k, (lin, f, c) in enumerate(real_frames(sc, setup)):
        got = device(lin, f, c, history=history, gamma=1.0)
        assert_same_outputs(got, host(lin, f, c, history=history, gamma=1.0), (k,))
        history = got
    assert got["clipped"].any() and ((got["length"] == 2.0) & (got["clipped"] == 0)).any()
    assert np.isfinite(got["sd"]).all() and np.isfinite(got["variance"]).all()


# ---- the handle

def composed(state, linear, features, cam, kw, clamp):
    """The header's composition with a clamp set, made with the product's own entry points on the device: (outputs, the map, next state)."""
    f = {k: np.ascontiguousarray(features[k], dtype=np.float64) for k in ("albedo", "normal", "depth", "alpha")}
    divided = np.zeros(linear.shape, dtype=bool)
    c, A1 = linear, f["albedo"]
    if kw["demodulate"]:
        divided = (f["alpha"][..., None] != 0.0) & (f["albedo"] > 1e-3)
        with np.errstate(all="ignore"):
            c = np.where(divided, linear / f["albedo"], linear)
        A1 = np.ones_like(linear)
    t = dict(max_history=kw["max_history"], normal_min=kw["normal_min"], min_temporal=kw["min_temporal"], radius=kw["radius"])
    accumulate = render.temporal_variance if clamp is None else (lambda *a, **k: render.temporal_clamp(*a, gamma=clamp["gamma"], clamp_radius=clamp["radius"], **k))
    over = lambda first: None if state is None else {"linear": first, "moment2": state["M2"], "length": state["L"], "features": state["features"],
                                                     "cam": state["cam"]}
    tv = accumulate(c, f, cam, history=over(None if state is None else state["M1"]), **t)
    A, bits = tv["linear"], np.zeros(linear.shape[:2], dtype=np.uint8) if clamp is None else tv["clipped"].copy()
    if kw["feedback"] > 0 and state is not None:
        if clamp is None:
            over_h = render.temporal_accumulate(c, f, cam, history=dict(over(state["H"]), variance=None), max_history=kw["max_history"], normal_min=kw["normal_min"])
        else:
            over_h = accumulate(c, f, cam, history=over(state["H"]), **t)                 # step 2: the same call over H; only its colour is kept
            bits |= over_h["clipped"] << 4
        assert same(over_h["length"], tv["length"]) and same(over_h["prev_xy"], tv["prev_xy"])
        A = over_h["linear"]
    f1 = dict(f, albedo=A1)
    D, _, Dv = render.denoise(A, f1, iterations=kw["iterations"], variance=tv["variance"])
    H = render.denoise(A, f1, iterations=kw["feedback"], variance=tv["variance"])[0] if kw["feedback"] > 0 else tv["linear"]
    with np.errstate(all="ignore"):
        shown, accumulated = np.where(divided, D * f["albedo"], D), np.where(divided, A * f["albedo"], A)
    out = {"linear_rgb": shown, "accumulated_rgb": accumulated, "variance_rgb": tv["variance"], "filtered_variance_rgb": Dv, "length": tv["length"],
           "prev_xy": tv["prev_xy"], "moment1_rgb": tv["linear"], "moment2_rgb": tv["moment2"], "history_rgb": H}
    return out, bits, {"H": H, "M1": tv["linear"], "M2": tv["moment2"], "L": tv["length"], "features": f, "cam": cam}


def handle_case(feedback, demodulate):
    case = next(c for c in reversed(svgf_cases.CASES) if c[1] == feedback and c[2] == demodulate and c[0][0] == (70, 41) and not c[0][6])
    return case, svgf_cases.settings(case), [svgf_cases.first_frame(case)] + svgf_cases.chain(case)[1]


@pytest.mark.parametrize("feedback,demodulate", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_a_clamped_handle_equals_the_product_calls_composed(gpu, feedback, demodulate):
    """70x41, the made-up history as a first frame, then three frames: every output the composition has, and both nibbles of the map."""
    case, kw, frames = handle_case(feedback, demodulate)
    clamp = {"gamma": 1.0, "radius": 3}
    state, low, high = None, 0, 0
    with render.SvgfSequence(70, 41, **kw) as seq:
        seq.set_clamp(**clamp)
        assert not seq.clipped().any()                                       # all 0 before a frame
        for k, (lin, f, cam) in enumerate(frames):
            got = seq.push(lin, f, cam)
            want, bits, state = composed(state, np.ascontiguousarray(lin), f, cam, kw, clamp)
            for name, arr in want.items():
                assert same(got[name], arr), (name, k)
            assert same(got["rgba8"], render.quantise_rgba8(want["linear_rgb"])), k
            assert np.array_equal(seq.clipped(), bits), k
            low, high = low + int((bits & 7 != 0).sum()), high + int((bits >> 4 != 0).sum())
    assert low > 0 and (high > 0) == (feedback > 0), (low, high)


def test_gamma_inf_on_the_handle_is_the_unclamped_handle(gpu):
    for feedback, demodulate in ((0, 1), (1, 0)):
        case, kw, frames = handle_case(feedback, demodulate)
        with render.SvgfSequence(70, 41, **kw) as a, render.SvgfSequence(70, 41, **kw) as b:
            a.set_clamp(gamma=INF, radius=4)
            for k, (lin, f, cam) in enumerate(frames):
                got, want = a.push(lin, f, cam), b.push(lin, f, cam)
                for name in render.SVGF_ARRAYS:
                    assert same(got[name], want[name]), (name, k)
                assert not a.clipped().any() and not b.clipped().any()


def test_set_clamp_keeps_the_history_and_clear_clamp_returns(gpu):
    """Unclamped for two frames, clamped for one, unclamped again: each frame equals the composition from the same state, and the map follows."""
    case, kw, frames = handle_case(1, 1)
    clamp = {"gamma": 0.25, "radius": 1}
    state = None
    with render.SvgfSequence(70, 41, **kw) as seq:
        for k, (lin, f, cam) in enumerate(frames):
            on = k == 2
            if on:
                seq.set_clamp(**clamp)
            elif k == 3:
                seq.clear_clamp()
            got = seq.push(lin, f, cam)
            want, bits, state = composed(state, np.ascontiguousarray(lin), f, cam, kw, clamp if on else None)
            for name, arr in want.items():
                assert same(got[name], arr), (name, k)
            assert np.array_equal(seq.clipped(), bits) and bits.any() == on, k
            if on:
                assert (got["length"] > 1.0).any()                           # the history was kept


def test_frame_with_a_clamp_on_cornell_box(scenes):
    """45x37, spp 2, three cameras 2 degrees apart: rttnw_svgf_frame with a clamp is rttnw_svgf_push of the two entry points' outputs on a second
    clamped handle; render_sequence_device(clamp=...) runs the same frames."""
    sc, setup = scenes["cornell_box"]
    cam, p = S.params_for(setup, 45, 37, 2, precision=abi.F64)
    cams = render.orbit_cameras(cam, 3, 2.0)
    sequence = render.render_sequence_device(sc, cams, p, feedback=1, demodulate=True, clamp=1.0)
    with render.SvgfSequence(45, 37, feedback=1, demodulate=True) as a, render.SvgfSequence(45, 37, feedback=1, demodulate=True) as b:
        a.set_clamp(gamma=1.0)
        b.set_clamp(gamma=1.0)
        for k, c in enumerate(cams):
            pk, pf = copy.copy(p), copy.copy(p)
            pk.sample_begin = pf.sample_begin = k * p.spp
            pf.spp = min(p.spp, 16)
            got = a.frame(sc, c, pk)
            raw, f = render.render_host(sc, c, pk)[0], render.render_features(sc, c, pf)
            assert same(got["raw_rgb"], raw), k
            want = b.push(raw, f, c)
            for name in render.SVGF_ARRAYS:
                assert same(got[name], want[name]), (name, k)
            assert np.array_equal(a.clipped(), b.clipped()) and np.array_equal(sequence[k]["clipped"], a.clipped()), k
            assert same(sequence[k]["linear"], got["linear_rgb"]), k
    assert a_clipped_something(sequence)


def a_clipped_something(sequence):
    return any((fr["clipped"] & 7).any() for fr in sequence[1:]) and any((fr["clipped"] >> 4).any() for fr in sequence[1:])


def test_cli_writes_the_python_composition(scenes, tmp_path):
    out = tmp_path / "image.png"
    r = subprocess.run([sys.executable, "-m", "rttnw_amd", "7", "--width", "64", "--spp", "4", "--orbit", "3", "--svgf", "--clamp", "1", "--out", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)   # a fresh child process
    assert r.returncode == 0, r.stderr
    assert "3 frames of 4 spp" in r.stdout and "the history clipped at gamma 1" in r.stdout and "svgf: feedback 0, colour" in r.stdout
    from PIL import Image
    sc, setup = scenes["cornell_box"]
    cam, p = S.params_for(setup, 64, 64, 4, precision=abi.F64)
    want = render.render_sequence_device(sc, render.orbit_cameras(cam, 3, 1.0), p, clamp=1.0)
    plain = render.render_sequence_device(sc, render.orbit_cameras(cam, 3, 1.0), p)
    host_side = render.render_sequence(sc, render.orbit_cameras(cam, 3, 1.0), p, variance=True, denoise=True, clamp=1.0)
    for k in range(3):
        im = Image.open(tmp_path / ("frame_%03d.png" % k))
        im.load()
        assert np.array_equal(np.asarray(im), want[k]["rgba8"]), k
        assert same(host_side[k]["linear"], want[k]["linear"]), k          # render_sequence(clamp=...) is the same loop with the host between its stages
    assert np.array_equal(want[0]["rgba8"], plain[0]["rgba8"]) and not np.array_equal(want[2]["rgba8"], plain[2]["rgba8"])
    assert "clipped" in host_side[2]["accumulated"] and "clipped" not in plain[2]
