"""rttnw_svgf_push and rttnw_svgf_frame on the MI355X: the device chain equals the numpy restatement of the header bit for bit, every field of
rttnw_svgf_out, on frames that cross the kernels' blocks; it equals the composition made with the product's own rttnw_temporal_variance,
rttnw_temporal_accumulate and rttnw_denoise calls; rttnw_svgf_frame is rttnw_svgf_push of rttnw_render's and rttnw_render_features' outputs, and
with feedback 0 and no demodulation render_sequence(variance=True, denoise=True); reset, independent handles, calls without outputs."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

import svgf_ref
from svgf_cases import CASE_IDS, CASES, ITERATIONS, assert_same_outputs, chain, check_chain, first_frame, settings
from temporal_cases import same
from rttnw_amd import abi, library, render
from rttnw_amd import scene as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Device(render.SvgfSequence):
    """render.SvgfSequence in the shape the shared checks take: push(linear, features, cam) -> every output."""


@pytest.fixture(scope="module")
def scenes(gpu):
    lib = library.scenes()
    return {name: S.build(gpu, lib, name) for name in ("cornell_box", "two_spheres")}


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_push_chains_equal_the_restatement_bit_for_bit(gpu, case):
    """The chains of tests/test_svgf_cpu.py, started from an empty handle with the made-up history as a first frame: 70x41 crosses the 64-wide
    blocks and is no multiple of 4 or 8 rows, 37 and 3 are no multiple of 8, 1x1 and 3x5 are smaller than a block and a tile."""
    check_chain(Device, svgf_ref.Restated, case, loaded=False)


@pytest.mark.parametrize("case", CASES[-12::4], ids=CASE_IDS[-12::4])
def test_two_handles_of_different_settings_alive_at_once(gpu, case):
    """Each link's frame goes through two handles, the case's settings and others, interleaved: each equals its own restatement."""
    (w, h) = case[0][0]
    kw = settings(case)
    other = dict(kw, feedback=(kw["feedback"] + 1) % 3, demodulate=not kw["demodulate"], radius=1 + kw["radius"] % 4)
    with Device(w, h, **kw) as a, Device(w, h, **other) as b:
        ra, rb = svgf_ref.Restated(w, h, **kw), svgf_ref.Restated(w, h, **other)
        for k, (lin, f, cam) in enumerate([first_frame(case)] + chain(case)[1]):
            ga, gb = a.push(lin, f, cam), b.push(lin, f, cam)
            assert_same_outputs(ga, ra.push(lin, f, cam), (k, "case"))
            assert_same_outputs(gb, rb.push(lin, f, cam), (k, "other"))


def composed(state, linear, features, cam, kw):
    """The header's composition with the product's own entry points on the device: (outputs, next state)."""
    f = {k: np.ascontiguousarray(features[k], dtype=np.float64) for k in ("albedo", "normal", "depth", "alpha")}
    divided = np.zeros(linear.shape, dtype=bool)
    c, A1 = linear, f["albedo"]
    if kw["demodulate"]:
        divided = (f["alpha"][..., None] != 0.0) & (f["albedo"] > 1e-3)
        with np.errstate(all="ignore"):
            c = np.where(divided, linear / f["albedo"], linear)
        A1 = np.ones_like(linear)
    t = dict(max_history=kw["max_history"], normal_min=kw["normal_min"])
    history = None if state is None else {"linear": state["M1"], "moment2": state["M2"], "length": state["L"], "features": state["features"], "cam": state["cam"]}
    tv = render.temporal_variance(c, f, cam, history=history, min_temporal=kw["min_temporal"], radius=kw["radius"], **t)
    A = tv["linear"]
    if kw["feedback"] > 0 and state is not None:
        over_h = render.temporal_accumulate(c, f, cam, history={"linear": state["H"], "variance": None, "length": state["L"], "features": state["features"],
                                                                "cam": state["cam"]}, **t)
        assert same(over_h["length"], tv["length"]) and same(over_h["prev_xy"], tv["prev_xy"])
        A = over_h["linear"]
    f1 = dict(f, albedo=A1)
    D, _, Dv = render.denoise(A, f1, iterations=kw["iterations"], variance=tv["variance"])
    H = render.denoise(A, f1, iterations=kw["feedback"], variance=tv["variance"])[0] if kw["feedback"] > 0 else tv["linear"]
    with np.errstate(all="ignore"):
        shown, accumulated = np.where(divided, D * f["albedo"], D), np.where(divided, A * f["albedo"], A)
    out = {"linear_rgb": shown, "accumulated_rgb": accumulated, "variance_rgb": tv["variance"], "filtered_variance_rgb": Dv, "length": tv["length"],
           "prev_xy": tv["prev_xy"], "moment1_rgb": tv["linear"], "moment2_rgb": tv["moment2"], "history_rgb": H}
    return out, {"H": H, "M1": tv["linear"], "M2": tv["moment2"], "L": tv["length"], "features": f, "cam": cam}


@pytest.mark.parametrize("feedback,demodulate", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_push_equals_the_product_calls_composed(gpu, feedback, demodulate):
    """One case per setting, 70x41: this pins the restatement to the product."""
    case = next(c for c in reversed(CASES) if c[1] == feedback and c[2] == demodulate)
    (w, h) = case[0][0]
    kw = settings(case)
    state = None
    with Device(w, h, **kw) as seq:
        for k, (lin, f, cam) in enumerate([first_frame(case)] + chain(case)[1]):
            got = seq.push(lin, f, cam)
            want, state = composed(state, np.ascontiguousarray(lin), f, cam, kw)
            for name, arr in want.items():
                assert same(got[name], arr), (name, k)
            assert same(got["rgba8"], render.quantise_rgba8(want["linear_rgb"])), k


def frame_calls(sc, cam, p, feature_spp=None):
    """What rttnw_svgf_frame renders, through the two entry points it joins."""
    pf = copy.copy(p)
    pf.spp = min(p.spp, 16) if feature_spp is None else feature_spp
    raw, _, st = render.render_host(sc, cam, p)
    return raw, render.render_features(sc, cam, pf), st


def orbit_params(setup, w, h, spp, precision, frames, step):
    cam, p = S.params_for(setup, w, h, spp, precision=precision)
    out = []
    for k, c in enumerate(render.orbit_cameras(cam, frames, step)):
        pk = copy.copy(p)
        pk.sample_begin = k * spp
        out.append((c, pk))
    return p, out


@pytest.mark.parametrize("precision", [abi.F64, abi.F32], ids=["f64", "f32"])
def test_frame_on_cornell_box(scenes, precision):
    """45x37, spp 2, four cameras 2 degrees apart: raw_rgb and the maps are the two entry points' outputs, everything else rttnw_svgf_push of them on
    a second handle; with feedback 0 and no demodulation the frames are render_sequence(variance=True, denoise=True)'s."""
    sc, setup = scenes["cornell_box"]
    p, frames = orbit_params(setup, 45, 37, 2, precision, 4, 2.0)
    want = render.render_sequence(sc, [c for c, _ in frames], p, variance=True, denoise=True)
    with Device(45, 37) as a, Device(45, 37) as b:
        for k, (cam, pk) in enumerate(frames):
            got = a.frame(sc, cam, pk)
            raw, f, st = frame_calls(sc, cam, pk)
            assert same(got["raw_rgb"], raw), k
            for name in ("albedo", "normal", "depth", "alpha"):
                assert same(got[name], f[name]), (name, k)
            assert_same_outputs(got, b.push(raw, f, cam), (k,))
            assert same(got["linear_rgb"], want[k]["linear"]) and same(got["rgba8"], want[k]["rgba8"]), k
            assert got["stats"].samples == st.samples + f["stats"].samples == 45 * 37 * 4
            assert got["image_ms"] > 0.0
    device = render.render_sequence_device(sc, [c for c, _ in frames], p)
    for k in range(4):
        assert same(device[k]["linear"], want[k]["linear"]) and same(device[k]["rgba8"], want[k]["rgba8"]) and same(device[k]["raw"], want[k]["raw"]), k
        assert same(device[k]["accumulated"]["variance"], want[k]["accumulated"]["variance"]), k


def test_frame_on_a_textured_scene_with_demodulation_and_feedback(scenes):
    """two_spheres (the checker texture), 45x37, spp 2, two frames, f64, feature_spp 3: the same equalities, and against the restatement."""
    sc, setup = scenes["two_spheres"]
    p, frames = orbit_params(setup, 45, 37, 2, abi.F64, 2, 2.0)
    kw = dict(feedback=1, demodulate=True, iterations=ITERATIONS)
    ref = svgf_ref.Restated(45, 37, **kw)
    with Device(45, 37, feature_spp=3, **kw) as a, Device(45, 37, **kw) as b:
        for k, (cam, pk) in enumerate(frames):
            got = a.frame(sc, cam, pk)
            raw, f, st = frame_calls(sc, cam, pk, feature_spp=3)
            assert same(got["raw_rgb"], raw), k
            for name in ("albedo", "normal", "depth", "alpha"):
                assert same(got[name], f[name]), (name, k)
            assert_same_outputs(got, b.push(raw, f, cam), (k,))
            assert_same_outputs(got, ref.push(raw, f, cam), (k, "restatement"))
            assert got["stats"].samples == 45 * 37 * 5
        assert (f["albedo"].max(axis=(0, 1)) - f["albedo"].min(axis=(0, 1))).max() > 0.3          # there is a texture in view
        assert (got["length"] == 2.0).mean() > 0.5


def test_reset_and_independence(gpu):
    """After reset the next call is a first frame's; two handles of different sizes do not disturb each other; calls with out == NULL and with
    only rgba8 asked for advance the state identically — seen through the following frame."""
    case, small = CASES[-1], CASES[40]                                    # 70x41 and 37x29
    (w, h), (sw, sh) = case[0][0], small[0][0]
    assert (w, h) != (sw, sh)
    kw = settings(case)
    frames = [first_frame(case)] + chain(case)[1]
    small_frames = [first_frame(small)] + chain(small)[1]
    with Device(w, h, **kw) as a, Device(sw, sh, **settings(small)) as s, Device(w, h, **kw) as quiet, Device(w, h, **kw) as rgba_only:
        ra, rs = svgf_ref.Restated(w, h, **kw), svgf_ref.Restated(sw, sh, **settings(small))
        for k in range(3):
            got = a.push(*frames[k])
            assert_same_outputs(s.push(*small_frames[k]), rs.push(*small_frames[k]), (k, "small"))
            assert_same_outputs(got, ra.push(*frames[k]), (k,))
            quiet.push(*frames[k], no_outputs=True)
            only = rgba_only.push(*frames[k], want=("rgba8",))
            assert same(only["rgba8"], got["rgba8"]) and set(only) == {"rgba8", "image_ms", "cam"}
        last = a.push(*frames[3])
        assert_same_outputs(quiet.push(*frames[3]), last, ("after calls without outputs",))
        assert_same_outputs(rgba_only.push(*frames[3]), last, ("after calls with rgba8 alone",))
        a.reset()
        fresh = svgf_ref.Restated(w, h, **kw)
        assert_same_outputs(a.push(*frames[2]), fresh.push(*frames[2]), ("after reset",))
        assert_same_outputs(a.push(*frames[3]), fresh.push(*frames[3]), ("the frame after",))


def test_frame_refuses_another_size_than_the_handles(scenes):
    """The one refusal that needs a handle (tests/test_svgf_abi_cpu.py has the others)."""
    sc, setup = scenes["cornell_box"]
    cam, p = S.params_for(setup, 45, 37, 2, precision=abi.F64)
    with Device(45, 36) as seq:
        with pytest.raises(abi.RttnwError, match="svgf_frame: p->width and p->height must equal the handle's"):
            seq.frame(sc, cam, p)


def test_cli_writes_the_device_chain(scenes, tmp_path):
    out = tmp_path / "image.png"
    r = subprocess.run([sys.executable, "-m", "rttnw_amd", "7", "--width", "64", "--spp", "4", "--orbit", "3", "--svgf", "--feedback", "1", "--demodulate",
                        "--out", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300)   # a fresh child process
    assert r.returncode == 0, r.stderr
    assert "3 frames of 4 spp" in r.stdout and "svgf: feedback 1, colour / albedo" in r.stdout
    from PIL import Image
    sc, setup = scenes["cornell_box"]
    cam, p = S.params_for(setup, 64, 64, 4, precision=abi.F64)
    want = render.render_sequence_device(sc, render.orbit_cameras(cam, 3, 1.0), p, feedback=1, demodulate=True)
    plain = render.render_sequence_device(sc, render.orbit_cameras(cam, 3, 1.0), p)
    for k in range(3):
        im = Image.open(tmp_path / ("frame_%03d.png" % k))
        im.load()
        assert np.array_equal(np.asarray(im), want[k]["rgba8"]), k
    assert not np.array_equal(want[2]["rgba8"], plain[2]["rgba8"])                         # the settings reached the loop
