"""rttnw_render_adaptive on the MI355X, held to its contract (include/rttnw_hip.h): pass 0 is the plain render, every pixel is the
composition of plain renders over its sample ranges, the noise estimate is the sample standard error, the stopping rule holds pixel by
pixel and does not depend on the cap or the launch split, and the estimate is calibrated."""
import copy
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_cases import build_scenes, use_kernel
from rttnw_amd import abi, render
from rttnw_amd import scene as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = [abi.F64, abi.F32, abi.F64_STRICT]
RTOL = {abi.F64: 1e-12, abi.F64_STRICT: 1e-12, abi.F32: 1e-5}
# refinement passes run the active-list form of the scene's kernel: the lane-owns-path one for these small scenes, the decoupled one
# (which larger scenes take) when RTTNW_KERNEL=wave forces it
KERNELS = [None, "wave"]


class AdaptivePixel(C.Structure):
    """rt::AdaptivePixel (rttnw_amd/csrc/adaptive.hpp)."""
    _fields_ = [("mu", C.c_double * 3), ("m2", C.c_double * 3), ("n", C.c_uint32), ("k", C.c_uint32)]


@pytest.fixture(scope="module")
def host():
    """The host build of the estimator the kernels include (tests/adaptive_host)."""
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "adaptive_host"), "-s"], check=True)
    lib = C.CDLL(os.path.join(ROOT, "tests", "adaptive_host", "libadaptive_host.so"))
    lib.ah_fold.argtypes = [C.POINTER(AdaptivePixel), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    lib.ah_fold.restype = None
    lib.ah_stderr.argtypes = [C.POINTER(AdaptivePixel), C.c_int]
    lib.ah_stderr.restype = C.c_double
    lib.ah_active.argtypes = [C.POINTER(AdaptivePixel), C.c_void_p, C.c_double, C.c_double, C.c_uint32]
    lib.ah_active.restype = C.c_int
    return lib


@pytest.fixture(scope="module")
def scenes(gpu):
    return build_scenes(gpu, ("cornell_box", "simple_light", "final_scene"))


def _params(scenes, name, w, spp, precision, **kw):
    sc, setup = scenes[name]
    cam, p = S.params_for(setup, w, w, spp, precision=precision, **kw)
    return sc, cam, p


def _plain(sc, cam, p, spp, begin):
    q = copy.copy(p)
    q.spp, q.sample_begin = spp, begin
    lin, rgba, _ = render.render_host(sc, cam, q, want_stats=False)
    return lin, rgba


@pytest.mark.parametrize("precision", PRECISIONS)
def test_pass0_is_the_plain_render(scenes, precision):
    sc, cam, p = _params(scenes, "cornell_box", 32, 32, precision, spp_chunk=2)
    lin, rgba, spp, se, st = render.render_adaptive(sc, cam, p, pass_spp=32, rel_error=0.0)
    lin0, rgba0 = _plain(sc, cam, p, 32, 0)
    assert np.array_equal(lin, lin0) and np.array_equal(rgba, rgba0)
    assert (spp == 32).all() and st.samples == 32 * 32 * 32
    assert np.isfinite(se).all()


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["cornell_box", "final_scene"])
def test_pixels_compose_from_plain_passes(scenes, name, precision, kernel, monkeypatch):
    use_kernel(monkeypatch, kernel)
    B, cap = 16, 64
    sc, cam, p = _params(scenes, name, 32, cap, precision, spp_chunk=4)
    lin, rgba, spp, se, st = render.render_adaptive(sc, cam, p, pass_spp=B, rel_error=0.15, abs_error=0.01)
    assert set(np.unique(spp).tolist()) <= {B, 2 * B, 3 * B, 4 * B}
    assert len(np.unique(spp)) > 1, "the tolerance should stop some pixels and not others"
    assert st.samples == int(spp.sum())
    passes = [_plain(sc, cam, p, B, k * B)[0] for k in range(cap // B)]
    want = np.zeros_like(lin)
    for k in range(cap // B):
        want += np.where((spp > k * B)[..., None], B * passes[k], 0.0)
    want /= spp[..., None]
    tol = RTOL[precision]
    assert np.all(np.abs(lin - want) <= tol * np.maximum(np.abs(want), 1e-300) + (1e-12 if tol < 1e-6 else 1e-7)), np.abs(lin - want).max()
    one = spp == B
    assert np.array_equal(lin[one], passes[0][one])
    assert np.array_equal(rgba[one], _plain(sc, cam, p, B, 0)[1][one])


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_device_state_is_the_host_harness_bit_for_bit(scenes, host, precision, kernel, monkeypatch):
    """The kernels' noise state and stopping decisions are those of the host build of adaptive.hpp, bit for bit: chunks of 4 and 2
    samples (B = 6, spp_chunk = 4), two passes.  A chunk's mean is a plain render of that chunk alone (a division by a power of two,
    exact in either precision), and a pixel's value after pass 0 is the plain render of its first B samples."""
    use_kernel(monkeypatch, kernel)
    B, cap, rel, ab = 6, 12, 0.3, 0.002
    sc, cam, p = _params(scenes, "cornell_box", 16, cap, precision, spp_chunk=4)
    _, _, spp, se, _ = render.render_adaptive(sc, cam, p, pass_spp=B, rel_error=rel, abs_error=ab)
    chunks = [(0, 4), (4, 2), (6, 4), (10, 2)]
    means = [_plain(sc, cam, p, n, s)[0] for s, n in chunks]
    value0 = _plain(sc, cam, p, B, 0)[0]
    n = np.ascontiguousarray([c[1] for c in chunks], dtype=np.uint32)
    want_spp = np.zeros_like(spp)
    want_se = np.zeros_like(se)
    for y in range(16):
        for x in range(16):
            m = np.ascontiguousarray([means[c][y, x] for c in range(4)])
            st = AdaptivePixel()
            host.ah_fold(C.byref(st), m.ctypes.data, n.ctypes.data, 0, 2)
            v = np.ascontiguousarray(value0[y, x])
            if host.ah_active(C.byref(st), v.ctypes.data, rel, ab, cap):
                host.ah_fold(C.byref(st), m.ctypes.data, n.ctypes.data, 2, 4)
            want_spp[y, x] = st.n
            want_se[y, x] = [host.ah_stderr(C.byref(st), ch) for ch in range(3)]
    assert np.array_equal(spp, want_spp)
    assert (spp == B).any() and (spp == cap).any()
    assert np.array_equal(se, want_se), np.abs(se - want_se).max()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_stderr_is_the_sample_standard_error(scenes, precision):
    sc, cam, p = _params(scenes, "cornell_box", 32, 8, precision, spp_chunk=1)
    _, _, spp, se, _ = render.render_adaptive(sc, cam, p, pass_spp=8, rel_error=0.0)
    assert (spp == 8).all()
    x = np.stack([_plain(sc, cam, p, 1, s)[0] for s in range(8)])
    want = x.std(axis=0, ddof=1) / np.sqrt(8)
    assert np.all(np.abs(se - want) <= 1e-9 * want + 1e-15), np.abs(se - want).max()


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_stopping_rule_prefix_and_launch_split(scenes, precision, kernel, monkeypatch):
    use_kernel(monkeypatch, kernel)
    B, cap, rel, ab = 16, 128, 0.1, 0.005
    sc, cam, p = _params(scenes, "simple_light", 32, cap, precision, spp_chunk=2)
    lin, rgba, spp, se, st = render.render_adaptive(sc, cam, p, pass_spp=B, rel_error=rel, abs_error=ab)
    done = spp < cap
    bound = ab + rel * lin
    assert np.all((se <= bound * (1 + 1e-12) + 1e-300).all(axis=2) | ~done)
    assert done.any() and (~done).any()
    # a lower cap: min(n_q, c) samples, the same bits wherever n_q <= c
    c = 64
    q = copy.copy(p)
    q.spp = c
    lin_c, rgba_c, spp_c, se_c, _ = render.render_adaptive(sc, cam, q, pass_spp=B, rel_error=rel, abs_error=ab)
    assert np.array_equal(spp_c, np.minimum(spp, c))
    keep = spp <= c
    assert np.array_equal(lin_c[keep], lin[keep]) and np.array_equal(se_c[keep], se[keep]) and np.array_equal(rgba_c[keep], rgba[keep])
    # every pass split into one-chunk launches: the same bits
    monkeypatch.setenv("RTTNW_CHUNK_SUM_BUDGET", "1")
    lin_s, rgba_s, spp_s, se_s, st_s = render.render_adaptive(sc, cam, p, pass_spp=B, rel_error=rel, abs_error=ab)
    assert np.array_equal(lin_s, lin) and np.array_equal(rgba_s, rgba) and np.array_equal(spp_s, spp) and np.array_equal(se_s, se)
    assert st_s.samples == st.samples == int(spp.sum())


@pytest.mark.parametrize("precision", PRECISIONS)
def test_stderr_is_calibrated(scenes, precision):
    # Uniform (one pass of the whole cap; with zero tolerances a pixel of zero variance would still stop early) against a 16384-sample
    # reference over a disjoint sample range.  Path-traced pixels are right-skewed: with few samples the rare bright paths are missing
    # from the mean and the variance alike, so the interval covers less than its 95 %.  Measured on cornell_box 64x64: 0.80 at 256
    # samples, 0.90 at 1024, 0.936 at 4096 — whatever the chunk size.  4096 samples is where the normal interval is tested.
    sc, cam, p = _params(scenes, "cornell_box", 64, 4096, precision, spp_chunk=256)
    lin, _, spp, se, _ = render.render_adaptive(sc, cam, p, pass_spp=4096, rel_error=0.0, abs_error=0.0)
    assert (spp == 4096).all()
    ref_p = copy.copy(p)
    ref_p.spp, ref_p.sample_begin, ref_p.spp_chunk = 16384, 1 << 20, 64
    ref, _, _, se_ref, _ = render.render_adaptive(sc, cam, ref_p, pass_spp=16384, rel_error=0.0)
    # (channels of zero variance in both — the light seen directly — carry no statistical information)
    random = (se > 0) | (se_ref > 0)
    assert random.mean() > 0.5
    inside = np.abs(lin - ref) <= 1.96 * np.sqrt(se ** 2 + se_ref ** 2)
    frac = inside[random].mean()
    print("calibration: %.4f of the pixel channels inside the 95 %% interval" % frac)
    assert 0.90 <= frac <= 0.98, frac


@pytest.mark.parametrize("precision", PRECISIONS)
def test_uneven_scene_traces_under_half(scenes, precision):
    sc, cam, p = _params(scenes, "simple_light", 64, 1024, precision, spp_chunk=4)
    _, _, spp, _, st = render.render_adaptive(sc, cam, p, pass_spp=64, rel_error=0.05, abs_error=0.0)
    full = 64 * 64 * 1024
    print("simple_light 64x64 cap 1024 rel 0.05: %d of %d samples (%.1f %%)" % (st.samples, full, 100.0 * st.samples / full))
    assert st.samples == int(spp.sum())
    assert st.samples < full / 2


def test_cli_writes_image_and_spp_map(gpu, tmp_path):
    out, smap = tmp_path / "img.png", tmp_path / "spp.png"
    r = subprocess.run([sys.executable, "-m", "rttnw_amd", "7", "--width", "48", "--spp", "128", "--pass-spp", "64", "--noise", "0.1",
                        "--out", str(out), "--spp-map", str(smap)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "samples traced of" in r.stdout
    from PIL import Image
    im, m = Image.open(out), Image.open(smap)
    assert im.size == (48, 48) and m.size == (48, 48) and m.mode == "L"
    v = np.asarray(m)
    assert v.min() >= 127 and v.max() == 255


def test_cli_rounds_the_default_cap_up(gpu, tmp_path):
    out = tmp_path / "img.png"
    r = subprocess.run([sys.executable, "-m", "rttnw_amd", "7", "--width", "32", "--noise", "0.2", "--out", str(out)], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "cap 200 spp rounded up to 256" in r.stdout and "of 262144 = 32x32x256" in r.stdout
    assert out.exists()
