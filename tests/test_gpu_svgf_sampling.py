"""rttnw_svgf_set_sampling and rttnw_svgf_samples on the MI355X: a frame call with sampling equals the composition the header writes down, made
with the product's own entry points — rttnw_render_region under the masks {m == level} of rttnw_svgf_samples' map composes the colour,
rttnw_render_features gives the maps, rttnw_svgf_push on a second handle takes both — in every field of rttnw_svgf_out, bit for bit; the map is
rttnw_temporal_probe's on the copied-out state; stats->samples counts what was traced; boost 1 and set_sampling(NULL) are an untouched handle.

The fill.  In the third frame (frame 2) of a sequence a reprojected length is at most 2, so k = floor(fill / (Lp + 1)) falls below 2 on a pixel
with a full history only for fill < 6: the cases that must show m == 1 and m > 1 on hit pixels in frame 2 run at fill 5 (a first frame gets 4
times the samples, the second 2 where it finds the first, the third 1 where it finds both).  At that fill a boost of 8 never reaches its level 8,
so three more cases run at the default fill of 8, where the frames' found pixels get 8, 4 and 2: there frame 2 must show levels 2 and 8."""
import copy
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from temporal_cases import same
from rttnw_amd import abi, library, render
from rttnw_amd import scene as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = H = 48
SPP, FRAMES, STEP = 2, 3, 2.0
PRECISIONS = {"f32": abi.F32, "f64": abi.F64, "f64strict": abi.F64_STRICT}
# (scene, boost, fill, precision, clamp gamma or None, handle settings)
CASES = [(name, boost, 5.0, prec, None, {}) for name in ("cornell_box", "final_scene") for boost in (4, 8) for prec in PRECISIONS]
CASES += [("cornell_box", 8, 5.0, "f64", 1.0, dict(feedback=1, demodulate=True)), ("final_scene", 4, 5.0, "f64", 1.0, dict(demodulate=True)),
          ("cornell_box", 8, 0.0, "f32", None, {}), ("final_scene", 8, 0.0, "f64", 1.0, dict(feedback=1, demodulate=True)),
          ("cornell_box", 8, 8.0, "f64strict", None, dict(demodulate=True))]
CASE_IDS = ["%s-b%d-f%g-%s%s%s" % (n, b, fl, pr, "-clamp" if g else "", "-" + "-".join(sorted(kw)) if kw else "") for n, b, fl, pr, g, kw in CASES]


@pytest.fixture(scope="module")
def scenes(gpu):
    lib = library.scenes()
    return {name: S.build(gpu, lib, name, S.load_earth() if name == "final_scene" else None) for name in ("cornell_box", "final_scene")}


def frame_params(p, k, stride):
    pk, pf = copy.copy(p), copy.copy(p)
    pk.sample_begin = pf.sample_begin = k * stride * p.spp
    pf.spp = min(p.spp, 16)
    return pk, pf


def composed_colour(sc, cam, pk, spp_map):
    """C of the header's step 3 on the host: per level present, rttnw_render_region under the mask {m == level} at level * spp."""
    colour, traced = np.zeros((H, W, 3)), 0
    for n in np.unique(spp_map):
        mask = spp_map == n
        pl = copy.copy(pk)
        pl.spp = int(n)
        lin, _, st = render.render_region(sc, cam, pl, 0, 0, W, H, mask=mask.astype(np.uint8))
        assert st.samples == int(mask.sum()) * int(n)
        colour[mask] = lin[mask]
        traced += int(mask.sum()) * int(n)
    return colour, traced


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_a_frame_with_sampling_equals_the_product_calls_composed(scenes, case):
    name, boost, fill, prec, gamma, kw = case
    sc, setup = scenes[name]
    cam, p = S.params_for(setup, W, H, SPP, precision=PRECISIONS[prec])
    levels_seen, state = [], None
    with render.SvgfSequence(W, H, **kw) as a, render.SvgfSequence(W, H, **kw) as b:
        assert a.set_sampling(boost=boost, fill=fill) == boost
        if gamma is not None:
            a.set_clamp(gamma=gamma)
            b.set_clamp(gamma=gamma)
        spp_map, length = a.samples()
        assert not spp_map.any() and not length.any()                        # before any frame call
        for k, c in enumerate(render.orbit_cameras(cam, FRAMES, STEP)):
            pk, pf = frame_params(p, k, boost)
            got = a.frame(sc, c, pk)
            spp_map, length = a.samples()
            f = render.render_features(sc, c, pf)
            for key in ("albedo", "normal", "depth", "alpha"):
                assert same(got[key], f[key]), (key, k)                     # F keeps its bits
            probe = render.temporal_probe(f, c, history=state, boost=boost, fill=fill)
            assert np.array_equal(spp_map, probe["multiplier"].astype(np.uint32) * SPP), k
            assert same(length, probe["length"]), k
            colour, traced = composed_colour(sc, c, pk, spp_map)
            assert same(got["raw_rgb"], colour), k
            want = b.push(colour, f, c)
            for key in render.SVGF_ARRAYS:
                assert same(got[key], want[key]), (key, k)
            if gamma is not None:
                assert np.array_equal(a.clipped(), b.clipped()), k
            # what was traced: the map's samples, the plain pass's discarded samples of the boosted pixels, the feature pass's rays
            discarded = int((spp_map > SPP).sum()) * SPP
            print("frame %d: traced %d + discarded %d + feature rays %d; levels %s" % (k, traced, discarded, W * H * pf.spp,
                                                                                         dict(zip(*np.unique(spp_map // SPP, return_counts=True)))))
            assert got["stats"].samples == traced + discarded + W * H * pf.spp, k
            assert got["stats"].kernel_ms > 0.0
            hit = f["alpha"] != 0.0
            m = spp_map // SPP
            assert np.all(m[~hit] == 1), k
            levels_seen.append(set(np.unique(m[hit]).tolist()))
            state = {"length": got["length"], "features": f, "cam": c}
    first = min(boost, 4 if fill == 5.0 else 8)
    assert levels_seen[0] == {first}, levels_seen
    if fill == 5.0:
        assert 1 in levels_seen[2] and max(levels_seen[2]) > 1, levels_seen   # frame 2: m == 1 and m > 1 on hit pixels
    else:
        assert {2, 8} <= levels_seen[2] and {4, 8} <= levels_seen[1], levels_seen


@pytest.mark.parametrize("name,prec", [("cornell_box", "f64"), ("final_scene", "f32")])
def test_boost_1_and_sampling_switched_off_are_an_untouched_handle(scenes, name, prec):
    """Three handles over the same frames: never touched, boost 1, and set then cleared before the first frame — every field of rttnw_svgf_out and,
    through the next frame, the state.  The map of the untouched ones is spp and zeros; boost 1 still probes, so its lengths are the probe's."""
    sc, setup = scenes[name]
    cam, p = S.params_for(setup, W, H, SPP, precision=PRECISIONS[prec])
    kw = dict(feedback=1, demodulate=True)
    state = None
    with render.SvgfSequence(W, H, **kw) as plain, render.SvgfSequence(W, H, **kw) as one, render.SvgfSequence(W, H, **kw) as cleared:
        one.set_sampling(boost=1, fill=100.0)
        cleared.set_sampling(boost=8)
        cleared.clear_sampling()
        for k, c in enumerate(render.orbit_cameras(cam, FRAMES, STEP)):
            pk, pf = frame_params(p, k, 1)
            want = plain.frame(sc, c, pk)
            for other in (one, cleared):
                got = other.frame(sc, c, pk)
                for key in render.SVGF_ARRAYS:
                    assert same(got[key], want[key]), (key, k)
                assert got["stats"].samples == want["stats"].samples == W * H * (SPP + pf.spp)
            for untouched in (plain, cleared):
                spp_map, length = untouched.samples()
                assert np.all(spp_map == SPP) and not length.any()
            spp_map, length = one.samples()
            f = {key: want[key] for key in ("albedo", "normal", "depth", "alpha")}
            assert np.all(spp_map == SPP) and same(length, render.temporal_probe(f, c, history=state, boost=1)["length"]), k
            assert (length > 0.0).any() == (k > 0)
            state = {"length": want["length"], "features": f, "cam": c}


def test_set_sampling_keeps_the_history_and_takes_effect_from_the_next_frame(scenes):
    """Plain for one frame, sampling for one, plain again: the middle frame's map is the probe's over the first frame's state (found pixels exist),
    and the third frame's is spp everywhere."""
    sc, setup = scenes["cornell_box"]
    cam, p = S.params_for(setup, W, H, SPP, precision=abi.F64)
    cams = render.orbit_cameras(cam, FRAMES, STEP)
    with render.SvgfSequence(W, H) as seq:
        first = seq.frame(sc, cams[0], frame_params(p, 0, 8)[0])
        seq.set_sampling(boost=8, fill=8.0)
        second = seq.frame(sc, cams[1], frame_params(p, 1, 8)[0])
        spp_map, length = seq.samples()
        f0 = {key: first[key] for key in ("albedo", "normal", "depth", "alpha")}
        f1 = {key: second[key] for key in ("albedo", "normal", "depth", "alpha")}
        probe = render.temporal_probe(f1, cams[1], history={"length": first["length"], "features": f0, "cam": cams[0]}, boost=8, fill=8.0)
        assert np.array_equal(spp_map, probe["multiplier"].astype(np.uint32) * SPP) and same(length, probe["length"])
        assert (length == 1.0).any() and (spp_map == 4 * SPP).any() and (second["length"] == 2.0).any()
        seq.clear_sampling()
        seq.frame(sc, cams[2], frame_params(p, 2, 8)[0])
        spp_map, length = seq.samples()
        assert np.all(spp_map == SPP) and not length.any()


def test_a_boost_times_spp_beyond_a_renders_spp_is_refused(scenes, gpu):
    sc, setup = scenes["cornell_box"]
    cam, p = S.params_for(setup, W, H, 2 ** 29, precision=abi.F64)
    with render.SvgfSequence(W, H) as seq:
        seq.set_sampling(boost=8)
        st = render.Stats()
        assert gpu.svgf_frame(seq.handle, sc.handle, C.byref(cam), C.byref(p), None, C.byref(st)) == -1
        err = gpu.last_error().decode()
        assert err.startswith("svgf_frame:") and "boost" in err and "spp" in err, err
        spp_map, _ = seq.samples()
        assert not spp_map.any()                                            # refused before anything ran


def test_render_sequence_device_and_the_command_line(scenes, tmp_path):
    """render_sequence_device(sampling=...) runs the handle's frames at sample_begin = k * boost * spp and returns the maps; the command line writes
    that sequence and one grey map a frame."""
    sc, setup = scenes["cornell_box"]
    cam, p = S.params_for(setup, 64, 64, 4, precision=abi.F64)
    cams = render.orbit_cameras(cam, 3, 1.0)
    sequence = render.render_sequence_device(sc, cams, p, sampling=(8, 5.0), want_spp=True)
    with render.SvgfSequence(64, 64) as seq:
        seq.set_sampling(boost=8, fill=5.0)
        for k, c in enumerate(cams):
            pk = copy.copy(p)
            pk.sample_begin = k * 8 * p.spp
            got = seq.frame(sc, c, pk)
            assert same(sequence[k]["linear"], got["linear_rgb"]) and np.array_equal(sequence[k]["spp"], seq.samples()[0]), k
    plain = render.render_sequence_device(sc, cams, p)
    assert "spp" not in plain[0] and not np.array_equal(plain[0]["rgba8"], sequence[0]["rgba8"])
    out = tmp_path / "image.png"
    r = subprocess.run([sys.executable, "-m", "rttnw_amd", "7", "--width", "64", "--spp", "4", "--orbit", "3", "--svgf", "--boost", "8", "--fill", "5",
                        "--spp-map", str(tmp_path / "spp_%03d.png"), "--out", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "sampling: boost 8, fill 5" in r.stdout and "3 frames of 4 spp" in r.stdout
    from PIL import Image
    for k in range(3):
        im = Image.open(tmp_path / ("frame_%03d.png" % k))
        im.load()
        assert np.array_equal(np.asarray(im), sequence[k]["rgba8"]), k
        grey = Image.open(tmp_path / ("spp_%03d.png" % k))
        grey.load()
        assert np.array_equal(np.asarray(grey), (sequence[k]["spp"].astype(np.uint64) * 255 // 32).astype(np.uint8)), k
