"""rttnw_render_region on the MI355X, held to its contract (include/rttnw_hip.h): a selected pixel is the full render's pixel bit for
bit — whatever the window, the mask, the precision, the kernel form, the launch split or the sample range — an unselected one is
0 / (0, 0, 0, 0), the oracle's own window and pixel-list calls agree with it, and it leaves the device state as the other renders
expect it.  Frames are 40x28: no multiple of 8 on either axis (partial tiles on both edges), 5x4 tiles (the tile rows' rotation)."""
import ctypes as C

import numpy as np
import pytest

from oracle import rto
from gpu_cases import build_scenes, use_kernel
from rttnw_amd import abi, library, render
from rttnw_amd import scene as S

pytestmark = pytest.mark.gpu
PRECISIONS = [abi.F64, abi.F32, abi.F64_STRICT]
KERNELS = [None, "wave"]   # the lane-owns-path list form these small scenes take, and the decoupled one RTTNW_KERNEL=wave forces
NAMES = ["cornell_box", "final_scene"]
W, H = 40, 28
WINDOWS = [(5, 3, 23, 18),     # odd edges: splits 2x2 blocks, crosses tile borders
           (0, 0, 40, 28),     # the whole frame
           (39, 27, 40, 28),   # one pixel, in the partial corner tile
           (6, 10, 8, 12),     # exactly one 2x2 block
           (7, 7, 9, 9)]       # four blocks of four tiles, one pixel each


@pytest.fixture(scope="module")
def scenes(gpu):
    return build_scenes(gpu, NAMES)


def _params(scenes, name, precision, spp=32, w=W, h=H, **kw):
    sc, setup = scenes[name]
    kw.setdefault("spp_chunk", 2)
    cam, p = S.params_for(setup, w, h, spp, precision=precision, **kw)
    return sc, cam, p


_FRAMES = {}


def _frame(scenes, name, precision, kernel, **kw):
    """The full frame of rttnw_render, rendered once per configuration (under the caller's RTTNW_KERNEL) and never written to."""
    key = (name, precision, kernel, tuple(sorted(kw.items())))
    if key not in _FRAMES:
        sc, cam, p = _params(scenes, name, precision, **kw)
        lin, rgba, st = render.render_host(sc, cam, p)
        lin.setflags(write=False)
        rgba.setflags(write=False)
        _FRAMES[key] = (lin, rgba, st.reserved, st.kernel_ms)
    return _FRAMES[key]


def _crop(a, win):
    x0, y0, x1, y1 = win
    return a[y0:y1, x0:x1]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", NAMES)
def test_a_window_is_the_crop_of_the_frame(scenes, name, precision, kernel, monkeypatch):
    use_kernel(monkeypatch, kernel)
    lin, rgba, form, _ = _frame(scenes, name, precision, kernel)
    sc, cam, p = _params(scenes, name, precision)
    for win in WINDOWS:
        x0, y0, x1, y1 = win
        l, r, st = render.render_region(sc, cam, p, *win)
        assert l.shape == (y1 - y0, x1 - x0, 3) and r.shape == (y1 - y0, x1 - x0, 4)
        assert np.array_equal(l, _crop(lin, win)), (win, np.abs(l - _crop(lin, win)).max())
        assert np.array_equal(r, _crop(rgba, win)), win
        assert (r[..., 3] == 255).all(), win
        assert st.samples == (x1 - x0) * (y1 - y0) * p.spp, win
        assert st.reserved == form and st.kernel_ms > 0 and st.n_nodes > 0, win


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", NAMES)
def test_a_mask_selects_pixels(scenes, name, precision, kernel, monkeypatch):
    use_kernel(monkeypatch, kernel)
    win = (2, 1, 38, 27)
    mask = np.random.default_rng(7).random((26, 36)) < 0.3
    assert 0 < mask.sum() < mask.size
    frame_sel = np.zeros((H, W), dtype=int)
    frame_sel[1:27, 2:38] = mask
    per_block = frame_sel.reshape(H // 2, 2, W // 2, 2).sum(axis=(1, 3))[1:13, 1:19]   # the 2x2 blocks that lie wholly inside the window
    assert (per_block == 1).any() and (per_block == 0).any()
    lin, rgba, _, _ = _frame(scenes, name, precision, kernel)
    sc, cam, p = _params(scenes, name, precision)
    l, r, st = render.render_region(sc, cam, p, *win, mask=mask)
    assert np.array_equal(l[mask], _crop(lin, win)[mask]) and np.array_equal(r[mask], _crop(rgba, win)[mask])
    assert (r[mask][:, 3] == 255).all()
    assert (l[~mask] == 0.0).all() and (r[~mask] == 0).all()
    assert st.samples == int(mask.sum()) * p.spp
    # nothing selected: no trace launch, cleared outputs
    b = library.product()
    l0 = np.full((26, 36, 3), 7.0)
    r0 = np.full((26, 36, 4), 7, dtype=np.uint8)
    zero = np.zeros((26, 36), dtype=np.uint8)
    st0 = abi.Stats()
    rc = b.render_region(sc.handle, C.byref(cam), C.byref(p), *win, zero.ctypes.data, l0.ctypes.data, r0.ctypes.data, C.byref(st0))
    assert rc == 0, b.last_error()
    assert (l0 == 0.0).all() and (r0 == 0).all() and st0.samples == 0
    l1, r1, st1 = render.render_region(sc, cam, p, *win, mask=np.zeros((26, 36), dtype=bool))
    assert (l1 == 0.0).all() and (r1 == 0).all() and st1.samples == 0


@pytest.mark.parametrize("precision", [abi.F64, abi.F32])
def test_an_empty_selection_reports_the_render_it_skipped(scenes, precision, monkeypatch):
    """A mask that selects nothing: no trace launch, so the stats come from a launch plan made for them alone — the kernel form (bits 0-5 of
    `reserved`) and the scene sizes must be those of a region render of the same scene and precision that did trace."""
    use_kernel(monkeypatch, None)
    win = (5, 3, 23, 18)
    sc, cam, p = _params(scenes, "cornell_box", precision, spp=4)
    _, _, traced = render.render_region(sc, cam, p, *win)
    l, r, st = render.render_region(sc, cam, p, *win, mask=np.zeros((15, 18), dtype=bool))
    assert (l == 0.0).all() and (r == 0).all() and st.samples == 0   # (alpha 0 as well)
    assert traced.samples == 15 * 18 * 4
    assert st.reserved & 0x3f == traced.reserved & 0x3f and st.n_nodes == traced.n_nodes > 0 and st.n_prims == traced.n_prims > 0


@pytest.fixture(scope="module")
def oracle_cornell(gpu, oracle, scenes_lib):
    """cornell_box 200x200 spp 50, default spp_chunk, RTTNW_F64_STRICT: the configuration test_config1_cornell_200_spp50_whole_frame holds
    whole, so the oracle is known to stay within the bound there."""
    sg, setup = S.build(gpu, scenes_lib, "cornell_box")
    so, _ = S.build(oracle, scenes_lib, "cornell_box")
    cam, p = S.params_for(setup, 200, 200, 50, precision=abi.F64_STRICT)
    return sg, so, cam, p


def test_the_oracles_own_window(oracle_cornell):
    sg, so, cam, p = oracle_cornell
    win = (37, 90, 101, 131)
    lo, ro, _, _ = rto.render_window(so, cam, p, *win)
    l, r, st = render.render_region(sg, cam, p, *win)
    d = np.abs(l - lo).max()
    print("region against rto.render_window: max abs difference %.3g" % d)
    assert d <= 1e-12
    assert np.array_equal(r, ro)
    assert st.samples == 64 * 41 * 50


def test_the_oracles_pixel_list(oracle_cornell):
    sg, so, cam, p = oracle_cornell
    x0, y0, x1, y1 = win = (37, 90, 101, 131)
    flat = np.random.default_rng(11).choice(64 * 41, size=12, replace=False)
    rows, cols = np.divmod(flat, 64)
    mask = np.zeros((41, 64), dtype=bool)
    mask[rows, cols] = True
    lo, ro, _ = rto.render_pixel_list(so, cam, p, x0 + cols, y0 + rows)
    l, r, st = render.render_region(sg, cam, p, *win, mask=mask)
    d = np.abs(l[rows, cols] - lo).max()
    print("region against rto.render_pixel_list: max abs difference %.3g" % d)
    assert d <= 1e-12
    assert np.array_equal(r[rows, cols], ro)
    assert (l[~mask] == 0.0).all() and (r[~mask] == 0).all() and st.samples == 12 * 50


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", NAMES)
def test_the_launch_split_changes_nothing(scenes, name, precision, monkeypatch):
    monkeypatch.delenv("RTTNW_KERNEL", raising=False)
    monkeypatch.delenv("RTTNW_CHUNK_SUM_BUDGET", raising=False)
    win = WINDOWS[0]
    sc, cam, p = _params(scenes, name, precision, spp=64)      # 32 chunks of 2
    l, r, st = render.render_region(sc, cam, p, *win)
    monkeypatch.setenv("RTTNW_CHUNK_SUM_BUDGET", "1")           # one-chunk launches
    l1, r1, st1 = render.render_region(sc, cam, p, *win)
    assert np.array_equal(l1, l) and np.array_equal(r1, r) and st1.samples == st.samples == 18 * 15 * 64
    monkeypatch.delenv("RTTNW_CHUNK_SUM_BUDGET")
    lin, rgba, _, _ = _frame(scenes, name, precision, None, spp=64)
    assert np.array_equal(l, _crop(lin, win)) and np.array_equal(r, _crop(rgba, win))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", NAMES)
def test_sample_ranges(scenes, name, precision, kernel, monkeypatch):
    use_kernel(monkeypatch, kernel)
    win = WINDOWS[0]
    lin, rgba, _, _ = _frame(scenes, name, precision, kernel, sample_begin=32)
    sc, cam, p = _params(scenes, name, precision, sample_begin=32)
    l, r, st = render.render_region(sc, cam, p, *win)
    assert np.array_equal(l, _crop(lin, win)) and np.array_equal(r, _crop(rgba, win))
    assert not np.array_equal(l, _crop(_frame(scenes, name, precision, kernel)[0], win))     # other samples than [0, 32)


def test_a_small_window_of_a_large_frame(scenes, monkeypatch):
    monkeypatch.delenv("RTTNW_KERNEL", raising=False)
    win = (392, 392, 408, 408)
    sc, cam, p = _params(scenes, "final_scene", abi.F64, spp=16, w=800, h=800, spp_chunk=0)
    lin, rgba, st_full = render.render_host(sc, cam, p)
    l, r, st = render.render_region(sc, cam, p, *win)
    print("final_scene 800x800 spp 16: full frame %.3f ms, 16x16 window %.3f ms" % (st_full.kernel_ms, st.kernel_ms))
    assert np.array_equal(l, _crop(lin, win)) and np.array_equal(r, _crop(rgba, win))
    assert st.samples == 256 * 16


@pytest.mark.parametrize("precision", PRECISIONS)
def test_back_to_back_on_one_scene(scenes, precision, monkeypatch):
    """The region render borrows the device state's buffers: it must not leave them in a state the other renders trip over, nor trip
    over what they leave."""
    monkeypatch.delenv("RTTNW_KERNEL", raising=False)
    win = WINDOWS[0]
    mask = np.random.default_rng(3).random((15, 18)) < 0.5
    sc, cam, p = _params(scenes, "final_scene", precision)
    full = render.render_host(sc, cam, p)[:2]
    adaptive = render.render_adaptive(sc, cam, p, pass_spp=16, rel_error=0.0)[:4]     # two passes, the second over a list of its own
    assert (adaptive[2] == 32).any()    # (a pixel without any noise, a black one, stops after the first)
    region = render.render_region(sc, cam, p, *win, mask=mask)[:2]
    assert np.array_equal(region[0][mask], _crop(full[0], win)[mask]) and (region[1][~mask] == 0).all()
    # ... and now one after the other
    region1 = render.render_region(sc, cam, p, *win, mask=mask)[:2]
    full1 = render.render_host(sc, cam, p)[:2]
    adaptive1 = render.render_adaptive(sc, cam, p, pass_spp=16, rel_error=0.0)[:4]
    region2 = render.render_region(sc, cam, p, *win, mask=mask)[:2]
    whole = render.render_region(sc, cam, p, 0, 0, W, H)[:2]
    for got, want in ((region1, region), (full1, full), (adaptive1, adaptive), (region2, region), (whole, full)):
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
