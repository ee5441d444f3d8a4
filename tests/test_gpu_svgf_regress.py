"""The regression stage of the rttnw_svgf handle on the MI355X (rttnw_svgf_set_regress / _push_halves / _halves): the device chain equals the
numpy restatement of the header bit for bit, every field of rttnw_svgf_out and of rttnw_svgf_halves, on frames that cross the kernels' blocks and
tiles; it equals the composition made with the product's own rttnw_temporal_variance, rttnw_temporal_accumulate (twice) and rttnw_denoise_regress
calls; the shared outputs are a plain handle's; without features the stage is rttnw_denoise_nlm; rttnw_svgf_frame is rttnw_svgf_push_halves of
two rttnw_render calls and rttnw_render_features; the lifecycle and every refusal that needs a handle; each rttnw_svgf_halves output alone; the
command line; and, recorded, what the stage does to the error against the converged oracle windows."""
import copy
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import svgf_ref
import svgf_regress_ref as R
from golden_cases import WINDOWS, load_windows
from svgf_cases import assert_same_outputs as assert_same_svgf_outputs
from temporal_cases import same
from rttnw_amd import abi, library, render
from rttnw_amd import scene as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HANDLE_KEYS = ("demodulate", "iterations", "sigma_luminance", "sigma_normal", "sigma_depth", "max_history", "depth_tolerance", "normal_min", "min_temporal",
               "radius", "variance_sigma_normal", "variance_sigma_depth", "feature_spp", "feedback")
STAGE_KEYS = ("mask", "ridge", "search_radius", "patch_radius", "k")


class Device(render.SvgfSequence):
    """render.SvgfSequence with the stage set, in the shape the shared checks take: push_halves(a, b, features, cam) -> every output of
    rttnw_svgf_out and of rttnw_svgf_halves."""

    def __init__(self, width, height, **kw):
        super().__init__(width, height, **{k: v for k, v in kw.items() if k in HANDLE_KEYS})
        stage = {k: v for k, v in kw.items() if k in STAGE_KEYS}
        self.set_regress(variance=render.REGRESS_VARIANCE[kw.get("variance_source", 0)], **dict({"mask": 7}, **stage))

    def push_halves(self, *args, **kw):
        out = super().push_halves(*args, **kw)
        out.update(self.halves())
        return out

    def frame(self, *args, **kw):
        out = super().frame(*args, **kw)
        out.update(self.halves())
        return out


@pytest.fixture(scope="module")
def scenes(gpu):
    lib = library.scenes()
    return {name: S.build(gpu, lib, name) for name in ("cornell_box",)}


# ---- 1: the restatement

@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_push_halves_chains_equal_the_restatement_bit_for_bit(gpu, case):
    """The chains of tests/test_svgf_regress_cpu.py: 45x37 is ragged against the 64x4 accumulate blocks and both filter tiles and crosses a
    32-pixel tile border on each axis, 70x9 crosses a 64-wide block border, 5x3 is smaller than every window."""
    R.check_chain(Device, R.Restated, case)


# ---- 2: the product's own entry points composed

def composed(state, a, b, features, cam, kw):
    """The header's composition with the product's own entry points on the device: (outputs, next state)."""
    f = {k: np.ascontiguousarray(features[k], dtype=np.float64) for k in ("albedo", "normal", "depth", "alpha")}
    C_ = (a + b) * 0.5
    divided = np.zeros(C_.shape, dtype=bool)
    c, ca, cb = C_, a, b
    if kw["demodulate"]:
        divided = (f["alpha"][..., None] != 0.0) & (f["albedo"] > 1e-3)
        with np.errstate(all="ignore"):
            c, ca, cb = (np.where(divided, x / f["albedo"], x) for x in (C_, a, b))
    history = None if state is None else {"linear": state["M1"], "moment2": state["M2"], "length": state["L"], "features": state["features"], "cam": state["cam"]}
    tv = render.temporal_variance(c, f, cam, history=history, min_temporal=kw["min_temporal"], radius=kw["radius"])
    Aa, Ab = ca, cb
    if state is not None:
        over = [render.temporal_accumulate(x, f, cam, history={"linear": state[H], "variance": None, "length": state["L"], "features": state["features"],
                                                               "cam": state["cam"]}) for x, H in ((ca, "Ha"), (cb, "Hb"))]
        for o in over:
            assert same(o["length"], tv["length"]) and same(o["prev_xy"], tv["prev_xy"])
        Aa, Ab = over[0]["linear"], over[1]["linear"]
    v2 = tv["variance"] + tv["variance"] if kw["variance_source"] == 0 else None
    r = render.denoise_regress(Aa, Ab, v2, v2, f, mask=kw["mask"], demodulate=False, search_radius=kw.get("search_radius", 0),
                               patch_radius=kw.get("patch_radius", 0))
    with np.errstate(all="ignore"):
        mean = (Aa + Ab) * 0.5
        shown, accumulated = np.where(divided, r["linear"] * f["albedo"], r["linear"]), np.where(divided, mean * f["albedo"], mean)
    out = {"linear_rgb": shown, "rgba8": render.quantise_rgba8(shown), "accumulated_rgb": accumulated, "variance_rgb": tv["variance"],
           "filtered_variance_rgb": r["error"], "length": tv["length"], "prev_xy": tv["prev_xy"], "moment1_rgb": tv["linear"], "moment2_rgb": tv["moment2"],
           "history_rgb": tv["linear"], "raw_rgb": C_, "albedo": f["albedo"], "normal": f["normal"], "depth": f["depth"], "alpha": f["alpha"], "acc_a": Aa,
           "acc_b": Ab, "filtered_a": r["half_a"], "filtered_b": r["half_b"], "fit": r["fit"]}
    return out, {"M1": tv["linear"], "M2": tv["moment2"], "Ha": Aa, "Hb": Ab, "L": tv["length"], "features": f, "cam": cam}


@pytest.mark.parametrize("case", [c for c in R.CASES if c[0] == R.SIZES[0] and c[1] == 1 and c[2] == 7 and not c[5]],
                         ids=lambda c: R.CASE_IDS[R.CASES.index(c)])
def test_a_chain_equals_the_public_entry_points_composed(gpu, case):
    """45x37, demodulated, every feature, both variance sources, with and without the NaN: this pins the restatement to the product.  Every output
    is compared, NaNs by position."""
    (w, h) = case[0]
    kw = R.settings(case)
    state = None
    with Device(w, h, **kw) as seq:
        for k, (a, b, f, cam) in enumerate(R.frames(case)):
            got = seq.push_halves(a, b, f, cam)
            want, state = composed(state, np.ascontiguousarray(a), np.ascontiguousarray(b), f, cam, kw)
            assert set(want) == set(R.OUTPUTS)
            for name, arr in want.items():
                assert np.array_equal(got[name], arr, equal_nan=arr.dtype == np.float64), (name, k)


# ---- 3, 4: the consequences

@pytest.mark.parametrize("demodulate", [0, 1])
def test_the_shared_outputs_equal_a_plain_handles_pushed_with_the_mean(gpu, demodulate):
    case = (R.SIZES[0], demodulate, 7, 0, False, False)
    (w, h) = case[0]
    kw = R.settings(case)
    with Device(w, h, **kw) as seq, render.SvgfSequence(w, h, feedback=0, demodulate=kw["demodulate"], min_temporal=kw["min_temporal"], radius=kw["radius"],
                                                        iterations=kw["iterations"]) as plain:
        for k, (a, b, f, cam) in enumerate(R.frames(case)):
            got, want = seq.push_halves(a, b, f, cam), plain.push((a + b) * 0.5, f, cam)
            for name in ("moment1_rgb", "moment2_rgb", "length", "prev_xy", "variance_rgb", "history_rgb", "raw_rgb", "albedo", "normal", "depth", "alpha"):
                assert same(got[name], want[name]), (name, k)
            assert not same(got["linear_rgb"], want["linear_rgb"]), k


@pytest.mark.parametrize("source", [0, 1], ids=["temporal", "pair"])
def test_without_features_linear_rgb_is_denoise_nlm_multiplied_back(gpu, source):
    case = (R.SIZES[0], 1, 0, source, False, False)
    (w, h) = case[0]
    with Device(w, h, **R.settings(case)) as seq:
        for k, (a, b, f, cam) in enumerate(R.frames(case)):
            got = seq.push_halves(a, b, f, cam)
            v2 = got["variance_rgb"] + got["variance_rgb"] if source == 0 else None
            want = render.denoise_nlm(got["acc_a"], got["acc_b"], v2, v2, **R.SMALL_RADII)
            divided = (f["alpha"][..., None] != 0.0) & (f["albedo"] > 1e-3)
            assert same(got["linear_rgb"], np.where(divided, want["linear"] * f["albedo"], want["linear"])), k
            assert same(got["filtered_a"], want["half_a"]) and same(got["filtered_b"], want["half_b"]) and same(got["filtered_variance_rgb"], want["error"]), k


# ---- 5: rttnw_svgf_frame

def orbit_params(setup, w, h, spp, precision, frames, step):
    cam, p = S.params_for(setup, w, h, spp, precision=precision)
    out = []
    for k, c in enumerate(render.orbit_cameras(cam, frames, step)):
        pk = copy.copy(p)
        pk.sample_begin = k * spp
        out.append((c, pk))
    return p, out


@pytest.mark.parametrize("precision", [abi.F64, abi.F32, abi.F64_STRICT], ids=["f64", "f32", "strict"])
def test_frame_is_push_halves_of_two_renders_and_the_feature_pass(scenes, precision):
    """cornell_box 45x37, spp 4, a 3-frame orbit at 2 degrees: the halves are rttnw_render's at spp 2 over the two sample ranges, the maps
    rttnw_render_features', and every output rttnw_svgf_push_halves' of them on a second handle; stats sums the two traces."""
    sc, setup = scenes["cornell_box"]
    _, frames = orbit_params(setup, 45, 37, 4, precision, 3, 2.0)
    kw = dict(demodulate=True, iterations=3, **R.SMALL_RADII)
    with Device(45, 37, **kw) as a, Device(45, 37, **kw) as b:
        for k, (cam, pk) in enumerate(frames):
            got = a.frame(sc, cam, pk)
            (ha, _, sta), (hb, _, stb) = render.render_halves(sc, cam, pk)
            f = render.render_features(sc, cam, pk)
            assert same(got["raw_rgb"], (ha + hb) * 0.5), k
            for name in ("albedo", "normal", "depth", "alpha"):
                assert same(got[name], f[name]), (name, k)
            R.assert_same_outputs(got, b.push_halves(ha, hb, f, cam), (k,))
            assert got["stats"].samples == sta.samples + stb.samples + f["stats"].samples == 45 * 37 * 8
            assert got["stats"].kernel_ms > 0.0
            assert got["image_ms"] > 0.0
        assert (got["length"] == 3.0).mean() > 0.5


# ---- 6: lifecycle

def test_every_exclusivity_refusal(scenes):
    sc, setup = scenes["cornell_box"]
    cam, p = S.params_for(setup, 45, 37, 4, precision=abi.F64)
    case = R.CASES[0]
    a, b, f, c0 = R.frames(case)[0]
    (w, h) = case[0]
    g = abi.Regress(features=7)
    lib = library.product()

    def refused(rc, call, msg):
        assert rc == -1, (call, rc)
        err = lib.last_error().decode()
        assert err.startswith(call + ":") and msg in err, err

    with render.SvgfSequence(w, h, feedback=1, iterations=3) as fed:
        refused(lib.svgf_set_regress(fed.handle, C.byref(g), 0), "svgf_set_regress", "exclusive with feedback_iterations != 0")
        assert lib.svgf_set_regress(fed.handle, None, 0) == 0                                    # clearing what is not set: a no-op
    with render.SvgfSequence(w, h, iterations=3) as seq:
        seq.set_clamp(gamma=1.0)
        refused(lib.svgf_set_regress(seq.handle, C.byref(g), 0), "svgf_set_regress", "exclusive with")
        seq.clear_clamp()
        seq.set_sampling(boost=2)
        refused(lib.svgf_set_regress(seq.handle, C.byref(g), 0), "svgf_set_regress", "exclusive with")
        seq.clear_sampling()
        # the order: g's own faults, then the stage's, come before the handle's state
        seq.set_clamp(gamma=1.0)
        refused(lib.svgf_set_regress(seq.handle, C.byref(abi.Regress(features=8)), 2), "svgf_set_regress", "g->features")
        refused(lib.svgf_set_regress(seq.handle, C.byref(abi.Regress(features=7, demodulate=1)), 2), "svgf_set_regress", "g->demodulate")
        refused(lib.svgf_set_regress(seq.handle, C.byref(g), 2), "svgf_set_regress", "variance_source")
        seq.clear_clamp()
        refused(lib.svgf_push_halves(seq.handle, C.byref(c0), *[np.ascontiguousarray(x).ctypes.data for x in (a, b, f["albedo"], f["normal"], f["depth"], f["alpha"])],
                                     None), "svgf_push_halves", "no regression stage")
        seq.set_regress(**R.SMALL_RADII)
        k = abi.Clamp(gamma=1.0)
        refused(lib.svgf_set_clamp(seq.handle, C.byref(k)), "svgf_set_clamp", "regression stage")
        refused(lib.svgf_set_sampling(seq.handle, C.byref(abi.Sampling(boost=2))), "svgf_set_sampling", "regression stage")
        assert lib.svgf_set_clamp(seq.handle, None) == 0 and lib.svgf_set_sampling(seq.handle, None) == 0     # a NULL block switches off what is off
        refused(lib.svgf_push(seq.handle, C.byref(c0), *[np.ascontiguousarray(x).ctypes.data for x in (a, f["albedo"], f["normal"], f["depth"], f["alpha"])], None),
                "svgf_push", "rttnw_svgf_push_halves")
        for spp in (3, 1):
            p.spp = spp
            refused(lib.svgf_frame(seq.handle, sc.handle, C.byref(cam), C.byref(p), None, None), "svgf_frame", "even and at least 2")
        p.spp = 4
        seq.frame(sc, cam, p, want=("rgba8",))                                                   # ... and the handle is none the worse for them
        seq.push_halves(a, b, f, c0, want=("rgba8",))


def test_set_then_clear_gives_the_bits_of_a_fresh_plain_handle(gpu):
    """Setting resets the history, clearing resets it again, and a NULL g on a handle without the stage keeps it."""
    case = (R.SIZES[0], 1, 7, 0, False, False)
    (w, h) = case[0]
    kw = dict(demodulate=True, iterations=3, min_temporal=2, radius=2)
    fr = R.frames(case)
    plain = [((a + b) * 0.5, f, cam) for a, b, f, cam in fr]
    with render.SvgfSequence(w, h, **kw) as seq, render.SvgfSequence(w, h, **kw) as fresh, render.SvgfSequence(w, h, **kw) as kept:
        seq.push(*plain[0])
        seq.set_regress(**R.SMALL_RADII)
        first = seq.push_halves(*fr[1])
        assert (first["length"] == 1.0).all()                                                    # set: a first frame
        for name in R.HALVES:
            assert seq.halves()[name].any(), name
        seq.push_halves(*fr[2])
        seq.clear_regress()
        for name in R.HALVES:
            assert not seq.halves()[name].any(), name                                            # all 0 again
        for k in (1, 2):
            assert_same_svgf_outputs(seq.push(*plain[k]), fresh.push(*plain[k]), (k,))           # clear: a fresh handle's bits
        kept.push(*plain[0])
        kept.clear_regress()                                                                     # nothing to clear: the history stays
        assert (kept.push(*plain[1])["length"] == 2.0).mean() > 0.3
        # a second set with other settings is a reset too, and takes the new settings
        seq.set_regress(mask=0, variance="pair", **R.SMALL_RADII)
        ref = R.Restated(w, h, **dict(R.settings(case), mask=0, variance_source=1))
        for k in (1, 2):
            got = seq.push_halves(*fr[k])
            got.update(seq.halves())
            R.assert_same_outputs(got, ref.push_halves(*fr[k]), (k, "set anew"))


def test_two_handles_of_different_stages_alive_at_once(gpu):
    """A plain handle, a regress handle and a non-local-means handle on the pair variance, fed the same frames interleaved: each equals its own
    restatement."""
    case = (R.SIZES[0], 1, 7, 0, False, False)
    (w, h) = case[0]
    kw = R.settings(case)
    other = dict(kw, mask=0, variance_source=1)
    plain_kw = dict(demodulate=True, iterations=3, min_temporal=2, radius=2)
    with Device(w, h, **kw) as a, render.SvgfSequence(w, h, **plain_kw) as p, Device(w, h, **other) as b:
        ra, rb, rp = R.Restated(w, h, **kw), R.Restated(w, h, **other), svgf_ref.Restated(w, h, **plain_kw)
        for k, (ha, hb, f, cam) in enumerate(R.frames(case)):
            ga, gp, gb = a.push_halves(ha, hb, f, cam), p.push((ha + hb) * 0.5, f, cam), b.push_halves(ha, hb, f, cam)
            R.assert_same_outputs(ga, ra.push_halves(ha, hb, f, cam), (k, "regress"))
            assert_same_svgf_outputs(gp, rp.push((ha + hb) * 0.5, f, cam), (k, "plain"))
            R.assert_same_outputs(gb, rb.push_halves(ha, hb, f, cam), (k, "nlm"))


# ---- 7: rttnw_svgf_halves' outputs one by one

GUARD, SENTINEL = 64, -12345.678


def test_each_halves_output_alone_equals_the_full_call_and_no_copy_leaves_its_array(gpu):
    case = R.CASES[0]
    (w, h) = case[0]
    sizes = [w * h * 3] * 4 + [w * h]

    def call(seq, wanted):
        arrays = [np.full(n + GUARD, SENTINEL) if i in wanted else None for i, n in enumerate(sizes)]
        assert gpu.svgf_halves(seq.handle, *[None if x is None else x.ctypes.data for x in arrays]) == 0, gpu.last_error().decode()
        return arrays

    with Device(w, h, **R.settings(case)) as seq:
        before = call(seq, range(5))                                                              # before any frame call: all 0, and no further
        for x, n in zip(before, sizes):
            assert not x[:n].any() and (x[n:] == SENTINEL).all()
        for fr in R.frames(case)[:2]:
            seq.push_halves(*fr, no_outputs=True)
        full = call(seq, range(5))
        for i, n in enumerate(sizes):
            alone = call(seq, [i])
            assert [x is not None for x in alone] == [j == i for j in range(5)]
            for x, what in ((full[i], "the full call"), (alone[i], "alone")):
                assert (x[n:] == SENTINEL).all(), (render.HALVES_ARRAYS[i], what, "wrote behind the array")
                assert not (x[:n] == SENTINEL).any(), (render.HALVES_ARRAYS[i], what, "left a value unwritten")
            assert full[i].tobytes() == alone[i].tobytes(), (render.HALVES_ARRAYS[i], "differs from the full call's")
        assert gpu.svgf_halves(seq.handle, None, None, None, None, None) == 0                     # nothing asked for: nothing done


# ---- 8: the command line

def test_cli_writes_the_device_chain(scenes, tmp_path):
    out = tmp_path / "image.png"
    r = subprocess.run([sys.executable, "-m", "rttnw_amd", "7", "--width", "64", "--spp", "4", "--orbit", "3", "--svgf", "--spatial", "regress",
                        "--fit-map", str(tmp_path / "fit_%03d.png"), "--out", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300)   # a fresh child process
    assert r.returncode == 0, r.stderr
    assert "3 frames of 4 spp" in r.stdout and "spatial stage: first-order regression over two accumulated halves" in r.stdout
    from PIL import Image
    sc, setup = scenes["cornell_box"]
    cam, p = S.params_for(setup, 64, 64, 4, precision=abi.F64)
    want = render.render_sequence_device(sc, render.orbit_cameras(cam, 3, 1.0), p, spatial="regress", want_halves=True)
    plain = render.render_sequence_device(sc, render.orbit_cameras(cam, 3, 1.0), p)
    for k in range(3):
        im = Image.open(tmp_path / ("frame_%03d.png" % k))
        im.load()
        assert np.array_equal(np.asarray(im), want[k]["rgba8"]), k
        fit = Image.open(tmp_path / ("fit_%03d.png" % k))
        fit.load()
        assert np.array_equal(np.asarray(fit), (want[k]["halves"]["fit"] * 127.5).astype(np.uint8)), k
    assert not np.array_equal(want[2]["rgba8"], plain[2]["rgba8"])                                # the stage reached the loop


# ---- 9: quality, recorded

QUALITY_SEQUENCES = [("plain", {}), ("regress, temporal", dict(spatial="regress", regress_variance="temporal")),
                     ("regress, pair", dict(spatial="regress", regress_variance="pair")), ("nlm, temporal", dict(spatial="nlm", regress_variance="temporal")),
                     ("nlm, pair", dict(spatial="nlm", regress_variance="pair"))]


@pytest.mark.parametrize("name", ["cornell_box", "final_scene"])
def test_quality_against_the_oracle_windows(gpu, name, capsys):
    """800x800, 4 spp, the 16-frame 1-degree orbit of profiles/clamp_measure.py, demodulate on: the MSE of the last frame against the committed
    t2_* oracle windows for the plain handle, the regress handle (every feature) and the non-local-means handle, the last two under both variance
    sources.  Asserted: every figure is finite, and in each window the regress handle's linear_rgb is closer to the oracle than the frame's own
    raw_rgb.  Everything else is printed: which stage wins where is a finding, not a gate."""
    sc, setup = S.build(gpu, library.scenes(), name, S.load_earth() if name == "final_scene" else None)
    cam, p = S.params_for(setup, 800, 800, 4, precision=abi.F64)
    cams = render.orbit_cameras(cam, 16, 1.0)
    gold = load_windows()
    last = {}
    for label, kw in QUALITY_SEQUENCES:
        frames = render.render_sequence_device(sc, cams, p, demodulate=True, want=("linear_rgb", "raw_rgb"), **kw)
        last[label] = (frames[-1]["linear"], frames[-1]["raw"], float(np.median([fr["image_ms"] for fr in frames[1:]])))
    windows = [(key, (slice(y0, y0 + ch), slice(x0, x0 + cw))) for key, scene, _, _, _, x0, y0, cw, ch, _ in WINDOWS if scene == name and key.startswith("t2_")]
    assert len(windows) == (3 if name == "cornell_box" else 4)
    figures = {}
    for key, crop in windows:
        ref = gold[key + "_linear"]
        figures[key] = {label: float(np.mean((lin[crop] - ref) ** 2)) for label, (lin, _, _) in last.items()}
        figures[key]["raw (regress handle)"] = float(np.mean((last["regress, temporal"][1][crop] - ref) ** 2))
        figures[key]["raw (regress handle, pair)"] = float(np.mean((last["regress, pair"][1][crop] - ref) ** 2))
    with capsys.disabled():
        for key, row in figures.items():
            print("\n%s MSE of frame 16 against the oracle window: %s" % (key, "; ".join("%s %.4g" % kv for kv in row.items())), flush=True)
        print("%s image_ms a frame (median of frames 2 - 16): %s" % (name, "; ".join("%s %.3f" % (label, v[2]) for label, v in last.items())), flush=True)
    for key, row in figures.items():
        assert all(np.isfinite(v) for v in row.values()), (key, row)
        assert row["regress, temporal"] < row["raw (regress handle)"], (key, row)
        assert row["regress, pair"] < row["raw (regress handle, pair)"], (key, row)
