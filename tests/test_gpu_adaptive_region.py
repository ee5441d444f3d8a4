"""rttnw_render_adaptive_region on the MI355X, held to its contract (include/rttnw_hip.h): a pixel this entry point selected and brought to the end
under a cap and tolerances is, bit for bit, that pixel of ONE fresh whole-frame adaptive render under them — linear value, RGBA8, sample count,
standard error and state record — whatever the window, the mask, the calls before it, the precision, the kernel form, the launch split and the
number of ranks on either side of a hand-over; an unselected pixel keeps its record, and a pixel without samples is zero everywhere, alpha included.
The reference F is always render.render_adaptive_resume(state=None) of the frame: code that existed before this entry point, never the entry point
itself.  One GPU, logical ranks: the device list repeats device 0.  The frames and parameters are those of tests/gpu_cases.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_cases import CASE1, CASE2, LOOSE_ABS, LOOSE_REL, build_scenes, fresh_cache, use_kernel
from gpu_cases import hist as _hist, same_outputs, samples as _samples, setup_case as _setup
from rttnw_amd import abi, render

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = [abi.F64, abi.F32, abi.F64_STRICT]
KERNELS = [None, "wave"]
RANKS = [None, [0, 0, 0]]
WINDOW = (3, 5, 30, 22)      # odd corners: aligned to neither the 2x2 blocks nor the 8x8 tiles; fits both frames
LEFT, OVERLAP = (0, 0, 25, 37), (17, 9, 45, 30)  # case 2: the left part of the frame, and a window that overlaps it and reaches the right edge


@pytest.fixture(scope="module")
def scenes(gpu):
    return build_scenes(gpu, ("cornell_box", "simple_light"))


def _frame(c):
    return (0, 0, c["w"], c["h"])


def _region(scenes, c, precision, win, mask=None, state=None, ids=None, **over):
    """One call of the entry point under test, under case c (with `over` laid over it): (linear, rgba8, spp, stderr, stats, state)."""
    c = dict(c, **over)
    sc, cam, p = _setup(scenes, c, precision)
    return render.render_adaptive_region(sc, cam, p, *win, mask=mask, state=state, device_ids=ids, pass_spp=c["B"], rel_error=c["rel"],
                                         abs_error=c["ab"])


@pytest.fixture(scope="module")
def fresh(scenes):
    """F: the uninterrupted whole-frame call of rttnw_render_adaptive_resume (state_in NULL, ngpu 0) per (case, precision, kernel form): computed
    once, shared, never written to."""
    def whole_frame(c, precision):
        sc, cam, p = _setup(scenes, c, precision)
        return render.render_adaptive_resume(sc, cam, p, None, None, pass_spp=c["B"], rel_error=c["rel"], abs_error=c["ab"])
    return fresh_cache(whole_frame)


def _crop(a, win):
    x0, y0, x1, y1 = win
    return a[y0:y1, x0:x1]


def _records(c, state):
    return state[64:].reshape(c["h"], c["w"], 12)


def _inside(c, win, mask=None):
    """The frame-sized boolean map of the pixels a call over (win, mask) selects."""
    sel = np.zeros((c["h"], c["w"]), dtype=bool)
    _crop(sel, win)[...] = True if mask is None else (np.asarray(mask) != 0)
    return sel


def _cleared(got, where, what=""):
    """A pixel without samples: 0, 0, 0, RGBA8 0, 0, 0, 0, spp 0, stderr 0."""
    assert not got[0][where].any() and not got[1][where].any() and not got[2][where].any() and not got[3][where].any(), what


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("ids", RANKS, ids=["ngpu0", "ranks3"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_whole_frame(scenes, fresh, precision, ids, kernel, monkeypatch):
    """Window = frame, no mask, no state: the four outputs and the state of F (level 0 runs over a list here, in the plain job numbering there),
    and exactly F's samples."""
    use_kernel(monkeypatch, kernel)
    ref = fresh(CASE2, precision, kernel)
    got = _region(scenes, CASE2, precision, _frame(CASE2), ids=ids)
    same_outputs(got, ref, what="whole frame")
    assert np.array_equal(got[5], ref[5], equal_nan=True), int((got[5] != ref[5]).sum())
    assert _samples(got[4]) == int(ref[2].sum())
    one = got[4][0] if ids else got[4]
    assert (one.reserved & ~0x300, one.n_nodes, one.n_prims, one.scene_bytes) == (ref[4].reserved, ref[4].n_nodes, ref[4].n_prims, ref[4].scene_bytes)
    assert one.kernel_ms > 0


@pytest.mark.parametrize("ids", RANKS, ids=["ngpu0", "ranks3"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_window(scenes, fresh, precision, ids):
    """Case 2, the window (3, 5)-(30, 22): every output is the crop of F, the state is F's inside the window and zero outside, and the call traced
    the crop's samples.  The crop holds more than one count, so more than one level ran.
    The crop's samples map on the MI355X, f64 (samples: pixels): {16: 280, 32: 7, 48: 5, 64: 167}."""
    ref = fresh(CASE2, precision)
    crop = [_crop(a, WINDOW) for a in ref[:4]]
    print("samples map of the crop: %s" % _hist(crop[2]))
    assert len(np.unique(crop[2])) >= 2, "more than one level must run"
    got = _region(scenes, CASE2, precision, WINDOW, ids=ids)
    same_outputs(got, crop, what="window")
    inside = _inside(CASE2, WINDOW)
    rec, ref_rec = _records(CASE2, got[5]), _records(CASE2, ref[5])
    assert np.array_equal(got[5][:64], ref[5][:64])
    assert np.array_equal(rec[inside], ref_rec[inside], equal_nan=True)
    assert not rec[~inside].any()
    assert _samples(got[4]) == int(crop[2].sum())


def _mask():
    x0, y0, x1, y1 = WINDOW
    return np.random.default_rng(7).random((y1 - y0, x1 - x0)) < 1.0 / 3.0


@pytest.mark.parametrize("ids", RANKS, ids=["ngpu0", "ranks3"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_mask(scenes, fresh, precision, ids):
    """A fixed pseudo-random third of that window: the selected pixels are F's, the others 0 with alpha 0, spp 0 and stderr 0 — in the outputs and
    in the state."""
    ref = fresh(CASE2, precision)
    crop = [_crop(a, WINDOW) for a in ref[:4]]
    mask = _mask()
    assert 0.25 < mask.mean() < 0.42
    got = _region(scenes, CASE2, precision, WINDOW, mask=mask, ids=ids)
    same_outputs(got, crop, where=mask, what="mask")
    assert (got[1][mask][:, 3] == 255).all()
    _cleared(got, ~mask, "unselected")
    inside = _inside(CASE2, WINDOW, mask)
    rec, ref_rec = _records(CASE2, got[5]), _records(CASE2, ref[5])
    assert np.array_equal(rec[inside], ref_rec[inside], equal_nan=True) and not rec[~inside].any()
    assert _samples(got[4]) == int(crop[2][mask].sum())


@pytest.mark.parametrize("ids", RANKS, ids=["ngpu0", "ranks3"])
def test_all_zero_mask(scenes, fresh, ids):
    """Nothing selected: RTTNW_OK, no sample traced; without a state the outputs are cleared and state_out is a header over zero records; with F's
    state the outputs are the state's own."""
    ref = fresh(CASE2, abi.F64)
    x0, y0, x1, y1 = WINDOW
    nothing = np.zeros((y1 - y0, x1 - x0), dtype=np.uint8)
    got = _region(scenes, CASE2, abi.F64, WINDOW, mask=nothing, ids=ids)
    assert _samples(got[4]) == 0
    _cleared(got, np.ones(nothing.shape, dtype=bool), "no state")
    assert np.array_equal(got[5][:64], ref[5][:64]) and not got[5][64:].any()
    got = _region(scenes, CASE2, abi.F64, WINDOW, mask=nothing, state=ref[5], ids=ids)
    assert _samples(got[4]) == 0
    same_outputs(got, [_crop(a, WINDOW) for a in ref[:4]], what="the state's own outputs")
    assert np.array_equal(got[5], ref[5], equal_nan=True)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_paint_then_complete(scenes, fresh, precision):
    """A on the left window into a state, B on an overlapping window with that state, C on the whole frame with that state: after C outputs and
    state are F's bit for bit, rttnw_render_adaptive_resume accepts the state and traces nothing, and A + B + C traced F's samples — none twice."""
    ref = fresh(CASE2, precision)
    ref_rec = _records(CASE2, ref[5])
    a = _region(scenes, CASE2, precision, LEFT)
    in_a = _inside(CASE2, LEFT)
    rec = _records(CASE2, a[5])
    assert not rec[~in_a].any() and np.array_equal(rec[in_a], ref_rec[in_a], equal_nan=True)
    same_outputs(a, [_crop(x, LEFT) for x in ref[:4]], what="A")
    sc, cam, p = _setup(scenes, CASE2, precision)
    with pytest.raises(abi.RttnwError, match="render_adaptive_resume: state_in: a record's n is below pass_spp"):
        render.render_adaptive_resume(sc, cam, p, a[5], None, pass_spp=CASE2["B"], rel_error=CASE2["rel"], abs_error=CASE2["ab"])
    b = _region(scenes, CASE2, precision, OVERLAP, state=a[5])
    in_ab = in_a | _inside(CASE2, OVERLAP)
    rec = _records(CASE2, b[5])
    assert not rec[~in_ab].any() and np.array_equal(rec[in_ab], ref_rec[in_ab], equal_nan=True)
    same_outputs(b, [_crop(x, OVERLAP) for x in ref[:4]], what="B")
    assert _samples(b[4]) == int(ref[2][in_ab & ~in_a].sum())
    c = _region(scenes, CASE2, precision, _frame(CASE2), state=b[5])
    same_outputs(c, ref, what="C")
    assert np.array_equal(c[5], ref[5], equal_nan=True)
    assert _samples(a[4]) + _samples(b[4]) + _samples(c[4]) == int(ref[2].sum())
    again = render.render_adaptive_resume(sc, cam, p, c[5], None, pass_spp=CASE2["B"], rel_error=CASE2["rel"], abs_error=CASE2["ab"])
    same_outputs(again, ref, what="resume of the completed state")
    assert again[4].samples == 0 and np.array_equal(again[5], ref[5], equal_nan=True)


@pytest.mark.parametrize("ids", RANKS, ids=["ngpu0", "ranks3"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_refine_where_you_look(scenes, fresh, precision, ids):
    """Case 1 at the loose tolerance (rel 0.5, abs 0.02) over the whole frame, then the window at case 1's own with that state: inside the window
    outputs and records are F's, outside the records are the loose state's; the pixels whose count grew started from at least two counts.  Then
    the same selection as a mask of a call over the whole frame: its outputs report the unselected pixels' loose values, with alpha 255.
    Samples maps of the window on the MI355X, f64 (samples: pixels), loose: {16: 427, 32: 9, 48: 12, 64: 4, 80: 4, 96: 2, 112: 1};
    case 1's own: {16: 403, 32: 2, 48: 3, 64: 1, 80: 2, 128: 48}."""
    ref = fresh(CASE1, precision)
    loose = fresh(CASE1, precision, rel=LOOSE_REL, ab=LOOSE_ABS)
    inside = _inside(CASE1, WINDOW)
    print("samples map of the window, loose: %s; tight: %s" % (_hist(_crop(loose[2], WINDOW)), _hist(_crop(ref[2], WINDOW))))
    grew = inside & (ref[2] > loose[2])
    assert grew.any() and len(np.unique(loose[2][grew])) >= 2, "pixels at more than one level must go on"
    got = _region(scenes, CASE1, precision, WINDOW, state=loose[5], ids=ids)
    same_outputs(got, [_crop(a, WINDOW) for a in ref[:4]], what="refined window")
    rec, ref_rec, loose_rec = _records(CASE1, got[5]), _records(CASE1, ref[5]), _records(CASE1, loose[5])
    assert np.array_equal(rec[inside], ref_rec[inside], equal_nan=True)
    assert np.array_equal(rec[~inside], loose_rec[~inside], equal_nan=True)
    assert _samples(got[4]) == int(ref[2][inside].sum()) - int(loose[2][inside].sum()) > 0
    masked = _region(scenes, CASE1, precision, _frame(CASE1), mask=inside, state=loose[5], ids=ids)
    same_outputs(masked, ref, where=inside, what="mask over the frame, selected")
    same_outputs(masked, loose, where=~inside, what="mask over the frame, unselected")
    assert (masked[1][..., 3] == 255).all()
    assert np.array_equal(masked[5], got[5], equal_nan=True)


@pytest.mark.parametrize("first,second", [(None, [0, 0, 0]), ([0, 0, 0], None)], ids=["0_then_3", "3_then_0"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_hand_over_between_rank_counts(scenes, fresh, precision, first, second):
    """A on one rank count, B and C on another: the same bits."""
    ref = fresh(CASE2, precision)
    a = _region(scenes, CASE2, precision, LEFT, ids=first)
    b = _region(scenes, CASE2, precision, OVERLAP, state=a[5], ids=second)
    same_outputs(b, [_crop(x, OVERLAP) for x in ref[:4]], what="B")
    c = _region(scenes, CASE2, precision, _frame(CASE2), state=b[5], ids=first)
    same_outputs(c, ref, what="C")
    assert np.array_equal(c[5], ref[5], equal_nan=True)
    assert _samples(a[4]) + _samples(b[4]) + _samples(c[4]) == int(ref[2].sum())


def test_peer_gather(scenes, fresh, monkeypatch):
    """... and the window once with the ranks' tiles gathered through peer copies."""
    ref = fresh(CASE2, abi.F64)
    monkeypatch.setenv("RTTNW_MULTI_GATHER", "peer")
    got = _region(scenes, CASE2, abi.F64, WINDOW, ids=[0] * 4)
    same_outputs(got, [_crop(a, WINDOW) for a in ref[:4]], what="peer")


def test_launch_split(scenes, fresh, monkeypatch):
    """The window of case 2 and its completion with every pass split into one-chunk launches (RTTNW_CHUNK_SUM_BUDGET=1)."""
    ref = fresh(CASE2, abi.F64)
    monkeypatch.setenv("RTTNW_CHUNK_SUM_BUDGET", "1")
    got = _region(scenes, CASE2, abi.F64, WINDOW)
    same_outputs(got, [_crop(a, WINDOW) for a in ref[:4]], what="one-chunk launches, window")
    done = _region(scenes, CASE2, abi.F64, _frame(CASE2), state=got[5])
    same_outputs(done, ref, what="one-chunk launches, completed")
    assert np.array_equal(done[5], ref[5], equal_nan=True)


def test_refusals_of_a_committed_scene(scenes, fresh):
    """A device id out of range and x1 > width name the entry point; the scene renders afterwards."""
    ref = fresh(CASE2, abi.F64)
    with pytest.raises(abi.RttnwError, match="render_adaptive_region: no such device"):
        _region(scenes, CASE2, abi.F64, WINDOW, ids=[0, -1])
    with pytest.raises(abi.RttnwError, match="render_adaptive_region: the window"):
        _region(scenes, CASE2, abi.F64, (3, 5, CASE2["w"] + 1, 22))
    got = _region(scenes, CASE2, abi.F64, WINDOW)
    same_outputs(got, [_crop(a, WINDOW) for a in ref[:4]], what="afterwards")


def test_cli_refine(gpu, tmp_path):
    """--refine of a window from nothing writes the window as the image: the crop of the one-shot adaptive run's PNG, pixel for pixel; and from
    that run's state, under the same rule, it traces nothing and writes the same window."""
    from PIL import Image
    base = [sys.executable, "-m", "rttnw_amd", "7", "--width", "40", "--noise", "0.1", "--pass-spp", "16", "--spp", "128"]
    one, win, again, state = (str(tmp_path / n) for n in ("one.png", "win.png", "again.png", "one.npy"))
    for argv in (["--save-state", state, "--out", one], ["--refine", "3,5,30,22", "--out", win],
                 ["--refine", "3,5,30,22", "--resume", state, "--devices", "0,0", "--out", again]):
        r = subprocess.run(base + argv, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert "samples traced of" in r.stdout
    assert "adaptive: 0 samples traced" in r.stdout
    crop = np.asarray(Image.open(one))[5:22, 3:30]
    assert np.array_equal(np.asarray(Image.open(win)), crop) and np.array_equal(np.asarray(Image.open(again)), crop)
    assert (crop[..., 3] == 255).all()
