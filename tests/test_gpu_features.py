"""rttnw_render_features on the MI355X, held to its contract (include/rttnw_hip.h): every feature value is the CPU oracle's, composed
sample by sample from its own operations (tests/features_ref.py), at the project's parity tiers; sample ranges compose; nothing depends
on the BVH builder, the frame's shape or the launch split."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

import features_ref
from oracle import rto
from rttnw_amd import abi, library, render
from rttnw_amd import scene as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = ["cornell_box", "simple_light", "final_scene", "two_perlin_spheres"]
KEYS = ("albedo", "normal", "depth", "alpha")
# The f32 build against the ORACLE on the eight frames of test_features_equal_the_oracle_sample_by_sample, over the pixels whose coverage
# equals the strict build's: the largest deviation measured on an MI355X per kind of channel (relative to max(1, |value|)), and the bound,
# 4x the measurement (headroom for a compiler update that rounds the f32 code differently).  Only the depth's is
# rounding (t |d| of an f32 ray over hundreds of units).  The normal's and the albedo's largest deviations are DECISIONS an f32 sample takes
# the other way, one sample of a pixel's four: a camera ray that differs by 2^-24 of its coordinates lands on the other side of an edge
# between two surfaces (both hits, so the coverage agrees: final_scene's cluster, 0.39 = a quarter of the difference of two unit
# normals), on the other side of a checker's sign change, or at another phase of a noise texture whose argument is in the hundreds.
F32_MEASURED = {"normal": 0.391, "albedo": 0.153, "depth": 4.19e-5}
F32_BOUND = {"normal": 1.564, "albedo": 0.612, "depth": 1.676e-4}


@pytest.fixture(scope="module")
def scenes(gpu):
    lib = library.scenes()
    out = {}
    for name in SCENES:
        earth = S.load_earth() if name == "final_scene" else None
        out[name] = (S.build(gpu, lib, name, earth), S.build(rto.binding(), lib, name, earth)[0])
    return out


_EXPECTED = {}


def _expected(scenes, name, w, h, spp, begin, cam=None):
    """The oracle's features of a frame, computed once per module."""
    key = (name, w, h, spp, begin, None if cam is None else (cam.open_time, cam.close_time))
    if key not in _EXPECTED:
        (_, setup), so = scenes[name]
        c, p = S.params_for(setup, w, h, spp, precision=abi.F64, sample_begin=begin)
        _EXPECTED[key] = features_ref.expected(so, cam if cam is not None else c, p)
    return _EXPECTED[key]


def _features(scenes, name, w, h, spp, begin, precision, cam=None):
    (sc, setup), _ = scenes[name]
    c, p = S.params_for(setup, w, h, spp, precision=precision, sample_begin=begin)
    return render.render_features(sc, cam if cam is not None else c, p)


@pytest.mark.parametrize("begin", [0, 7])
@pytest.mark.parametrize("name", SCENES)
def test_features_equal_the_oracle_sample_by_sample(scenes, name, begin):
    """64x64, spp 4.  On the CPU these eight frames have NO pixel whose first-hit decision (hit or miss, material, front face, scattered)
    changes when the oracle's camera ray is moved by 1e-12 in any coordinate (tests/features_ref.py expected(perturb=1e-12)), so the
    contracted build's 0.1 % allowance is not consumed by the frames themselves."""
    want = _expected(scenes, name, 64, 64, 4, begin)
    strict = _features(scenes, name, 64, 64, 4, begin, abi.F64_STRICT)
    d = features_ref.deviation(strict, want)
    print("%s begin %d strict: max deviation %.3g" % (name, begin, d.max()))
    assert np.array_equal(strict["alpha"], want["alpha"])
    assert d.max() <= 1e-12, (d.max(), np.argwhere(d > 1e-12)[:8])
    assert strict["stats"].samples == strict["stats"].rays == 64 * 64 * 4 and strict["stats"].kernel_ms > 0.0

    f64 = _features(scenes, name, 64, 64, 4, begin, abi.F64)
    d = features_ref.deviation(f64, want)
    beyond = np.argwhere(d > 1e-9)
    print("%s begin %d f64: max deviation %.3g, %d pixels beyond 1e-9 %s" % (name, begin, d.max(), len(beyond), beyond[:8].tolist()))
    assert (d <= 1e-9).mean() >= 0.999

    f32 = _features(scenes, name, 64, 64, 4, begin, abi.F32)
    same = f32["alpha"] == strict["alpha"]
    d = features_ref.deviation(f32, want)
    by_key = {k: float((np.abs(f32[k] - want[k]) / np.maximum(1.0, np.abs(want[k])))[same].max()) for k in KEYS}
    print("%s begin %d f32: coverage equal on %.4f of the pixels; largest deviation on those %.3g %s"
          % (name, begin, same.mean(), d[same].max(), by_key))
    print("%s begin %d f32: share of those pixels within 1e-3 of the oracle in every channel %.4f" % (name, begin, (d[same] <= 1e-3).mean()))
    assert same.mean() >= 0.999
    for k in ("normal", "albedo", "depth"):
        assert by_key[k] <= F32_BOUND[k], (k, by_key[k])


@pytest.mark.parametrize("precision,tol", [(abi.F64_STRICT, 1e-12), (abi.F64, 1e-12), (abi.F32, 2e-6)])
def test_sample_ranges_compose(scenes, precision, tol):
    """Features over [0, 3) and [3, 8) combine, with weights 3 and 5, to the features over [0, 8).  (f32: the two chains round differently,
    eight additions of 2^-24 relative each.)"""
    for name in ("cornell_box", "final_scene"):
        a = _features(scenes, name, 48, 48, 3, 0, precision)
        b = _features(scenes, name, 48, 48, 5, 3, precision)
        whole = _features(scenes, name, 48, 48, 8, 0, precision)
        for k in KEYS:
            comb = (3.0 * a[k] + 5.0 * b[k]) / 8.0
            e = np.abs(comb - whole[k]) / np.maximum(1.0, np.abs(whole[k]))
            assert e.max() <= tol, (name, k, e.max())


def test_the_bvh_builder_does_not_change_the_features(gpu):
    lib = library.scenes()
    outs = []
    for bvh in (abi.BVH_HOST_SAH, abi.BVH_DEVICE_LBVH, abi.BVH_DEVICE_SAH):
        sc, setup = S.build(gpu, lib, "final_scene", S.load_earth(), bvh=bvh)
        cam, p = S.params_for(setup, 64, 64, 4, precision=abi.F64_STRICT)
        outs.append(render.render_features(sc, cam, p))
    for other in outs[1:]:
        for k in KEYS:
            assert np.array_equal(other[k], outs[0][k]), k


def test_a_ragged_frame(scenes):
    want = _expected(scenes, "final_scene", 45, 37, 2, 0)
    got = _features(scenes, "final_scene", 45, 37, 2, 0, abi.F64_STRICT)
    assert got["albedo"].shape == (37, 45, 3) and got["depth"].shape == (37, 45)
    assert np.array_equal(got["alpha"], want["alpha"]) and features_ref.deviation(got, want).max() <= 1e-12
    assert features_ref.deviation(_features(scenes, "final_scene", 45, 37, 2, 0, abi.F64), want).max() <= 1e-9


def test_a_shutter_outside_the_trees_interval_rebuilds_them(gpu, oracle):
    """tests/graph_shapes.py wide_shutter: moving spheres seen through a shutter of [-0.5, 1.7].  The first call rebuilds the trees for
    that interval (include/rttnw_hip.h, the conventions; BvhTree::from_time, hittable.rs:261), and the features are still the oracle's."""
    import graph_shapes
    sg = S.Scene(gpu, 7)
    sg.set_world(graph_shapes.SHAPES["wide_shutter"](sg))
    sg.commit()
    so, cam, p = graph_shapes.build(oracle, "wide_shutter", w=48, h=36, spp=3, precision=abi.F64_STRICT)
    assert cam.open_time < 0.0 and cam.close_time > 1.0
    before = sg.build_info().lower_ms
    got = render.render_features(sg, cam, p)
    want = features_ref.expected(so, cam, p)
    assert np.array_equal(got["alpha"], want["alpha"]) and features_ref.deviation(got, want).max() <= 1e-12
    assert sg.build_info().lower_ms != before                      # (the rebuild's own wall time has replaced the commit's)
    p64 = copy.copy(p)
    p64.precision = abi.F64
    assert (features_ref.deviation(render.render_features(sg, cam, p64), want) <= 1e-9).mean() >= 0.999


def test_the_launch_split_changes_nothing(scenes, monkeypatch):
    base = {pr: _features(scenes, "cornell_box", 64, 64, 4, 0, pr) for pr in (abi.F64, abi.F32, abi.F64_STRICT)}
    monkeypatch.setenv("RTTNW_CHUNK_SUM_BUDGET", "1")
    for pr, want in base.items():
        got = _features(scenes, "cornell_box", 64, 64, 4, 0, pr)
        for k in KEYS:
            assert np.array_equal(got[k], want[k]), (pr, k)


def test_cli_writes_the_denoised_image_and_the_feature_maps(gpu, tmp_path):
    out = tmp_path / "image.png"
    r = subprocess.run([sys.executable, "-m", "rttnw_amd", "7", "--width", "96", "--spp", "8", "--denoise", "--features", str(tmp_path / "x"),
                        "--out", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300)   # a fresh child process
    assert r.returncode == 0, r.stderr
    assert "denoised: 5 iterations" in r.stdout
    from PIL import Image
    im = Image.open(out)
    im.load()
    assert im.size == (96, 96) and im.mode == "RGBA"
    for suffix, mode in (("albedo", "RGBA"), ("normal", "RGB"), ("depth", "L"), ("alpha", "L")):
        m = Image.open(tmp_path / ("x_%s.png" % suffix))
        m.load()
        assert m.size == (96, 96) and m.mode == mode, suffix
    assert np.asarray(Image.open(tmp_path / "x_alpha.png")).max() == 255
    assert np.asarray(Image.open(tmp_path / "x_depth.png")).max() == 255
