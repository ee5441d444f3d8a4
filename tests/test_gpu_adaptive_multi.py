"""rttnw_render_adaptive_multi on the MI355X, held to its contract (include/rttnw_hip.h): the linear image, the RGBA8, the samples map and the
standard-error map are rttnw_render_adaptive's bit for bit — for every number of ranks, precision, kernel form, launch split and gather
transport — and the ranks' samples add up to the single call's.  One GPU, logical ranks: the device list repeats device 0."""
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_cases import CASE1, CASE2, build_scenes, fresh_cache, use_kernel
from gpu_cases import setup_case as _setup
from rttnw_amd import abi, render, tiles

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = [abi.F64, abi.F32, abi.F64_STRICT]
KERNELS = [None, "wave"]
# (case 1 and case 2: tests/gpu_cases.py)
# the tolerance of test_a_rank_that_finishes_early: of 8 ranks over case 1's frame, two stop after their first pass and the others after their
# 2nd .. 7th (the samples of each rank's slowest pixel on the single-GPU result: 80, 16, 112, 80, 32, 48, 96, 16)
EARLY_REL, EARLY_ABS = 0.5, 0.02


@pytest.fixture(scope="module")
def scenes(gpu):
    return build_scenes(gpu, ("cornell_box", "simple_light"))


def _single(scenes, c, precision):
    sc, cam, p = _setup(scenes, c, precision)
    return render.render_adaptive(sc, cam, p, pass_spp=c["B"], rel_error=c["rel"], abs_error=c["ab"])


@pytest.fixture(scope="module")
def single(scenes):
    """rttnw_render_adaptive's result per (case, precision, kernel form): computed once, shared by the tests, never written to."""
    return fresh_cache(lambda c, precision: _single(scenes, c, precision))


def _multi(scenes, c, precision, n):
    sc, cam, p = _setup(scenes, c, precision)
    return render.render_adaptive_multi(sc, cam, p, [0] * n, pass_spp=c["B"], rel_error=c["rel"], abs_error=c["ab"])


def _assert_same(got, ref, c, n):
    """The four outputs bit for bit (+inf equal to +inf, NaN to NaN), the ranks' samples, and device time on every rank that owns a tile."""
    lin, rgba, spp, se, sts = got
    lin0, rgba0, spp0, se0, st0 = ref
    assert np.array_equal(lin, lin0), (n, np.abs(lin - lin0).max())
    assert np.array_equal(rgba, rgba0), n
    assert np.array_equal(spp, spp0), (n, int((spp != spp0).sum()))
    assert np.array_equal(se, se0, equal_nan=True), n
    assert len(sts) == n
    assert sum(x.samples for x in sts) == int(spp0.sum()) == st0.samples, n
    owner, _ = tiles.packed_index(c["w"], c["h"], n)
    for r, x in enumerate(sts):
        assert x.samples == int(spp0[owner == r].sum()), (n, r)                 # each rank traced the samples of ITS pixels
        if (owner == r).any():
            assert x.kernel_ms > 0, (n, r)
            assert (x.reserved & 0xFF) == (st0.reserved & 0xFF) and (x.n_nodes, x.n_prims, x.scene_bytes) == (st0.n_nodes, st0.n_prims, st0.scene_bytes)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_bit_identity_over_ranks(scenes, single, precision, kernel, monkeypatch):
    """Case 1 (simple_light 40x24, B = 16, cap = 128, rel_error 0.1, abs_error 0.005, spp_chunk 2) over 1, 2, 3 and 8 logical ranks.  The
    single-GPU result must hold pixels that stopped after the first pass, pixels at the cap and pixels in between, or the equalities
    would say little."""
    use_kernel(monkeypatch, kernel)
    ref = single(CASE1, precision, kernel)
    values = set(np.unique(ref[2]).tolist())
    print("samples map of the single call: %s" % dict(zip(*np.unique(ref[2], return_counts=True))))
    assert CASE1["B"] in values and CASE1["cap"] in values and any(CASE1["B"] < v < CASE1["cap"] for v in values), values
    for n in (1, 2, 3, 8):
        _assert_same(_multi(scenes, CASE1, precision, n), ref, CASE1, n)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_frame_not_a_multiple_of_8(scenes, single, precision):
    """Case 2 (cornell_box 45x37, B = 16, cap = 64, rel_error 0.15, abs_error 0.01, spp_chunk 4) over 4 and 7 ranks: edge tiles reach outside
    the image, and 7 ranks leave pad tiles."""
    ref = single(CASE2, precision)
    assert len(np.unique(ref[2])) > 1, "the tolerance should stop some pixels and not others"
    for n in (4, 7):
        _assert_same(_multi(scenes, CASE2, precision, n), ref, CASE2, n)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_launch_split(scenes, single, precision, monkeypatch):
    """Case 1 over 3 ranks with every pass split into one-chunk launches (RTTNW_CHUNK_SUM_BUDGET=1): the same bits."""
    ref = single(CASE1, precision)
    monkeypatch.setenv("RTTNW_CHUNK_SUM_BUDGET", "1")
    _assert_same(_multi(scenes, CASE1, precision, 3), ref, CASE1, 3)


def test_a_rank_that_finishes_early(scenes, single):
    """Case 1 under a looser tolerance (rel_error 0.5, abs_error 0.02), 8 ranks: on the single-GPU result every pixel of at least one rank's
    tiles stopped after the first pass while another rank went on — so that rank leaves the pass loop before the others."""
    c = dict(CASE1, rel=EARLY_REL, ab=EARLY_ABS)
    ref = single(c, abi.F64)
    owner, _ = tiles.packed_index(c["w"], c["h"], 8)
    last = [int(ref[2][owner == r].max()) for r in range(8)]
    print("samples of each rank's slowest pixel: %s" % last)
    assert min(last) == c["B"] and max(last) > c["B"], last
    _assert_same(_multi(scenes, c, abi.F64, 8), ref, c, 8)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_ranks_that_finish_together_and_the_infinite_standard_error(scenes, single, precision):
    """Two edges of the pass loop, case 1's frame with ONE chunk per pass (spp_chunk = B), 3 ranks.  After the first pass a pixel has K = 1 chunk,
    so it cannot stop; with a tolerance nothing misses, every pixel of every rank stops after the second: all ranks leave the loop together,
    before the cap.  And with the cap at B the standard error of every pixel is +inf, which has to travel through the auxiliary records."""
    c = dict(CASE1, spp_chunk=CASE1["B"], cap=4 * CASE1["B"], rel=1e6, ab=1e6)
    ref = single(c, precision)
    assert (ref[2] == 2 * c["B"]).all() and np.isfinite(ref[3]).all()
    _assert_same(_multi(scenes, c, precision, 3), ref, c, 3)
    c = dict(c, cap=c["B"])
    ref = single(c, precision)
    assert (ref[2] == c["B"]).all() and np.isposinf(ref[3]).all()
    _assert_same(_multi(scenes, c, precision, 3), ref, c, 3)


_LEG_SCRIPT = r"""
import sys
sys.path.insert(0, %(root)r)
import numpy as np
from rttnw_amd import abi, library, render, scene as S
gpu, scenes = library.product(), library.scenes()
sc, setup = S.build(gpu, scenes, "simple_light")
cam, p = S.params_for(setup, 40, 24, 128, precision=abi.F64, spp_chunk=2)
one = render.render_adaptive(sc, cam, p, pass_spp=16, rel_error=0.1, abs_error=0.005)
got = render.render_adaptive_multi(sc, cam, p, [0, 0, 0], pass_spp=16, rel_error=0.1, abs_error=0.005)
assert len(np.unique(one[2])) > 2
assert np.array_equal(got[0], one[0]) and np.array_equal(got[1], one[1]) and np.array_equal(got[2], one[2])
assert np.array_equal(got[3], one[3], equal_nan=True)
assert sum(x.samples for x in got[4]) == one[4].samples
print("ADAPTIVE_LEG_OK bits=%%d" %% (int(got[4][0].reserved) & 0x300))
"""


def test_gather_transports_on_one_gpu(gpu, tmp_path):
    """The image and the auxiliary records through both gather transports and the fall-through, on one GPU: under
    RTTNW_MULTI_FORCE_TRANSPORT=1 the ranks on the root's device travel through the transport too (tests/test_gpu_parity.py
    test_render_multi_gather_transports_on_one_gpu says what each leg runs).  3 ranks on device 0, f64, case 1; one child process per leg,
    each with a time limit, and no leg starts after another has failed."""
    script = tmp_path / "adaptive_leg.py"
    script.write_text(_LEG_SCRIPT % {"root": ROOT})
    legs = [("rccl", {}, 0, "through ncclSend / ncclRecv"),
            ("peer", {"RTTNW_MULTI_GATHER": "peer"}, 0x100, "through hipMemcpyPeerAsync"),
            ("rccl_fails", {"RTTNW_MULTI_FAIL_RCCL": "1"}, 0x300, "RCCL gather unavailable (RTTNW_MULTI_FAIL_RCCL=1): gathering through peer copies")]
    for leg, extra, bits, line in legs:
        env = dict(os.environ, RTTNW_MULTI_FORCE_TRANSPORT="1", RTTNW_DEBUG_MULTI="1", **extra)
        r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "ADAPTIVE_LEG_OK bits=%d" % bits in r.stdout, (leg, r.stdout[-2000:], r.stderr[-4000:])
        assert line in r.stderr, (leg, r.stderr[-4000:])
        # two buffers per travelling rank: its packed tiles and its auxiliary records
        assert "6 rank buffer(s)" in r.stderr, (leg, r.stderr[-4000:])


def test_no_such_device(gpu, scenes):
    sc, cam, p = _setup(scenes, CASE1, abi.F64)
    with pytest.raises(abi.RttnwError, match="no such device"):
        render.render_adaptive_multi(sc, cam, p, [gpu.device_count()], pass_spp=CASE1["B"], rel_error=CASE1["rel"], abs_error=CASE1["ab"])
    with pytest.raises(abi.RttnwError, match="no such device"):
        render.render_adaptive_multi(sc, cam, p, [0, -1], pass_spp=CASE1["B"], rel_error=CASE1["rel"], abs_error=CASE1["ab"])


def test_cli_devices(gpu, tmp_path):
    """`--devices` with `--noise` goes through rttnw_render_adaptive_multi and writes the image and the map the same command writes without it."""
    from PIL import Image
    base = [sys.executable, "-m", "rttnw_amd", "7", "--width", "48", "--spp", "128", "--pass-spp", "64", "--noise", "0.1"]
    out, smap, out1, smap1 = (tmp_path / n for n in ("img.png", "spp.png", "img1.png", "spp1.png"))
    r = subprocess.run(base + ["--devices", "0,0,0", "--out", str(out), "--spp-map", str(smap)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "samples traced of" in r.stdout and "per rank:" in r.stdout
    line = [x for x in r.stdout.splitlines() if "samples traced of" in x][0]
    per_rank = [int(v) for v in line.split("per rank:")[1].rstrip(")").split()]
    assert len(per_rank) == 3 and sum(per_rank) == int(line.split("adaptive: ")[1].split()[0])
    r1 = subprocess.run(base + ["--out", str(out1), "--spp-map", str(smap1)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0, r1.stderr
    assert "per rank:" not in r1.stdout
    im = Image.open(out)
    assert im.size == (48, 48) and Image.open(smap).mode == "L"
    assert np.array_equal(np.asarray(im), np.asarray(Image.open(out1))) and np.array_equal(np.asarray(Image.open(smap)), np.asarray(Image.open(smap1)))


def test_cli_devices_without_noise(gpu, tmp_path):
    """`--devices` without `--noise` goes through rttnw_render_multi: the pixels of the same command without it."""
    from PIL import Image
    plain = [sys.executable, "-m", "rttnw_amd", "7", "--width", "48", "--spp", "32"]
    out2, out3 = tmp_path / "img2.png", tmp_path / "img3.png"
    r2 = subprocess.run(plain + ["--devices", "0,0,0", "--out", str(out2)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0 and "3 ranks" in r2.stdout, r2.stderr
    r3 = subprocess.run(plain + ["--out", str(out3)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r3.returncode == 0, r3.stderr
    assert np.array_equal(np.asarray(Image.open(out2)), np.asarray(Image.open(out3)))
