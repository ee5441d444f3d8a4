"""rttnw_render_adaptive_resume on the MI355X, held to its contract (include/rttnw_hip.h): a render continued from a state — to a higher cap, to a
tighter tolerance, step by step, on another number of ranks — is the render that was never interrupted, bit for bit: linear image, RGBA8, samples
map, standard-error map and the state itself.  One GPU, logical ranks: the device list repeats device 0.  The frames and parameters are those of
tests/gpu_cases.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import abi_cases
from gpu_cases import CASE1, CASE2, LOOSE_ABS, LOOSE_REL, build_scenes, fresh_cache, use_kernel
from gpu_cases import hist as _hist, same_outputs, samples as _samples, setup_case as _setup
from rttnw_amd import abi, render, tiles

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = [abi.F64, abi.F32, abi.F64_STRICT]
KERNELS = [None, "wave"]


@pytest.fixture(scope="module")
def scenes(gpu):
    return build_scenes(gpu, ("cornell_box", "simple_light"))


def _resume(scenes, c, precision, state=None, ids=None, **over):
    """One call under case c (with `over` laid over it): (linear, rgba8, spp, stderr, stats, state)."""
    c = dict(c, **over)
    sc, cam, p = _setup(scenes, c, precision)
    return render.render_adaptive_resume(sc, cam, p, state, ids, pass_spp=c["B"], rel_error=c["rel"], abs_error=c["ab"])


@pytest.fixture(scope="module")
def fresh(scenes):
    """The uninterrupted call (state_in NULL, ngpu 0) per (case, precision, kernel form): computed once, shared, never written to."""
    return fresh_cache(lambda c, precision: _resume(scenes, c, precision))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_fresh_equals_the_existing_calls(scenes, fresh, precision):
    """state_in NULL: rttnw_render_adaptive's four outputs with ngpu 0, and the same over three logical ranks — stats included."""
    sc, cam, p = _setup(scenes, CASE1, precision)
    one = render.render_adaptive(sc, cam, p, pass_spp=CASE1["B"], rel_error=CASE1["rel"], abs_error=CASE1["ab"])
    got = fresh(CASE1, precision)
    same_outputs(got, one, what="ngpu 0")
    assert got[4].samples == one[4].samples == int(one[2].sum())
    assert (got[4].reserved, got[4].n_nodes, got[4].n_prims, got[4].scene_bytes) == (one[4].reserved, one[4].n_nodes, one[4].n_prims, one[4].scene_bytes)
    assert got[4].kernel_ms > 0
    three = _resume(scenes, CASE1, precision, ids=[0, 0, 0])
    same_outputs(three, got, what="three ranks")
    assert len(three[4]) == 3 and _samples(three[4]) == one[4].samples


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_checkpoint(scenes, fresh, precision, kernel, monkeypatch):
    """Case 1 stopped at a cap of 48, then resumed to 128: the one fresh call with cap 128.  At 48 some pixels had converged and some stood at
    the cap; the final map goes beyond it, so the resumed call had real work, and it traced exactly the difference."""
    use_kernel(monkeypatch, kernel)
    ref = fresh(CASE1, precision, kernel)
    part = fresh(CASE1, precision, kernel, cap=48)
    print("samples map at cap 48: %s; at cap 128: %s" % (_hist(part[2]), _hist(ref[2])))
    assert (part[2] < 48).any() and (part[2] == 48).any() and (ref[2] > 48).any()
    got = _resume(scenes, CASE1, precision, state=part[5])
    same_outputs(got, ref, what="checkpoint")
    assert got[4].samples == int(ref[2].sum()) - int(part[2].sum()) > 0


@pytest.mark.parametrize("precision", PRECISIONS)
def test_refine(scenes, fresh, precision):
    """Case 1 at the loose tolerance (rel 0.5, abs 0.02), then resumed at its own (0.1, 0.005): a fresh case 1.  The pixels whose count grew
    started from at least two different counts — more than one level ran — and some pixel kept its count.
    Samples maps on the MI355X, f64 (samples: pixels), loose: {16: 919, 32: 12, 48: 15, 64: 5, 80: 6, 96: 2, 112: 1};
    case 1's own: {16: 893, 32: 2, 48: 3, 64: 1, 80: 3, 128: 58}."""
    ref = fresh(CASE1, precision)
    loose = fresh(CASE1, precision, rel=LOOSE_REL, ab=LOOSE_ABS)
    print("samples map, loose: %s; tight: %s" % (_hist(loose[2]), _hist(ref[2])))
    grew = ref[2] > loose[2]
    assert len(np.unique(loose[2][grew])) >= 2, "more than one level must run"
    assert (ref[2] == loose[2]).any(), "some pixel keeps its count"
    assert (ref[2] >= loose[2]).all()
    got = _resume(scenes, CASE1, precision, state=loose[5])
    same_outputs(got, ref, what="refine")
    assert got[4].samples == int(ref[2].sum()) - int(loose[2].sum())


def test_progressive(scenes, fresh):
    """Case 1 in eight calls with caps 16, 32, ..., 128, each from the state of the one before: the fresh cap-128 call, and the calls' samples
    add up to its."""
    ref = fresh(CASE1, abi.F64)
    state, traced, got = None, 0, None
    for cap in range(16, 129, 16):
        got = _resume(scenes, CASE1, abi.F64, state=state, cap=cap)
        state = got[5]
        traced += got[4].samples
    same_outputs(got, ref, what="progressive")
    assert traced == ref[4].samples == int(ref[2].sum())


def test_nothing_to_do(scenes, fresh):
    """A finished state resumed with unchanged arguments, and with a higher cap under a tolerance every pixel already meets: RTTNW_OK, no sample
    traced, the outputs of the call that made the state, the state unchanged."""
    ref = fresh(CASE1, abi.F64)
    got = _resume(scenes, CASE1, abi.F64, state=ref[5])
    same_outputs(got, ref, what="unchanged arguments")
    assert got[4].samples == 0
    part = fresh(CASE1, abi.F64, cap=48)
    got = _resume(scenes, CASE1, abi.F64, state=part[5], cap=256, rel=1e9, ab=1e9)
    same_outputs(got, part, what="tolerance 1e9")
    assert got[4].samples == 0
    ranks = _resume(scenes, CASE1, abi.F64, state=part[5], ids=[0, 0], cap=256, rel=1e9, ab=1e9)
    same_outputs(ranks, part, what="tolerance 1e9, two ranks")
    assert [x.samples for x in ranks[4]] == [0, 0]


def _per_rank(c, n, stats, before, after):
    owner, _ = tiles.packed_index(c["w"], c["h"], n)
    assert len(stats) == n
    for r, x in enumerate(stats):
        assert x.samples == int(after[owner == r].sum()) - int(before[owner == r].sum()), (n, r)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_across_rank_counts(scenes, fresh, precision):
    """Case 2 (45x37: edge tiles reach outside the image, 7 ranks leave pad tiles): a state made on the single device at cap 32 and resumed
    on 4 and on 7 ranks to cap 64, and a state made on 3 ranks resumed on the single device — all the fresh single call, and every rank traced
    the new samples of its own pixels."""
    ref = fresh(CASE2, precision)
    part = fresh(CASE2, precision, cap=32)
    assert (part[2] == 32).any() and (ref[2] > 32).any()
    for n in (4, 7):
        got = _resume(scenes, CASE2, precision, state=part[5], ids=[0] * n)
        same_outputs(got, ref, what="%d ranks" % n)
        _per_rank(CASE2, n, got[4], part[2], ref[2])
    part3 = _resume(scenes, CASE2, precision, ids=[0] * 3, cap=32)
    same_outputs(part3, part, what="state made on 3 ranks")
    got = _resume(scenes, CASE2, precision, state=part3[5])
    same_outputs(got, ref, what="3 ranks, then the single device")
    assert got[4].samples == int(ref[2].sum()) - int(part[2].sum())


def test_peer_gather(scenes, fresh, monkeypatch):
    """... and once with the ranks' tiles gathered through peer copies."""
    ref = fresh(CASE2, abi.F64)
    part = fresh(CASE2, abi.F64, cap=32)
    monkeypatch.setenv("RTTNW_MULTI_GATHER", "peer")
    got = _resume(scenes, CASE2, abi.F64, state=part[5], ids=[0] * 4)
    same_outputs(got, ref, what="peer")
    _per_rank(CASE2, 4, got[4], part[2], ref[2])


def test_launch_split(scenes, fresh, monkeypatch):
    """The checkpoint of case 1, f64, with every pass of the RESUMED call split into one-chunk launches (RTTNW_CHUNK_SUM_BUDGET=1)."""
    ref = fresh(CASE1, abi.F64)
    part = fresh(CASE1, abi.F64, cap=48)
    monkeypatch.setenv("RTTNW_CHUNK_SUM_BUDGET", "1")
    same_outputs(_resume(scenes, CASE1, abi.F64, state=part[5]), ref, what="one-chunk launches")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_state_says_what_the_outputs_say(fresh, precision):
    lin, rgba, spp, se, st, state = fresh(CASE1, precision)
    c = CASE1
    assert state.shape == (64 + 12 * c["w"] * c["h"],)
    head = state[:64]
    assert head[0] == abi_cases.MAGIC and head[1] == abi_cases.VERSION and (head[2], head[3], head[4], head[5]) == (c["w"], c["h"], c["B"], c["spp_chunk"])
    assert head[7] == precision and not head[31:].any()
    rec = state[64:].reshape(c["h"], c["w"], 12)
    n, k = rec[..., 3], rec[..., 7]
    assert np.array_equal(n, spp.astype(np.float64))
    assert np.array_equal(k, n / c["B"] * 8)                       # B = 16 in chunks of 2
    assert not rec[..., 11].any()
    many = k >= 2
    assert many.any()
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.array_equal(np.sqrt(rec[..., 8:11] / ((k - 1) * n)[..., None])[many], se[many])
    if precision == abi.F32:
        assert np.array_equal(rec[..., 0:3].astype(np.float32).astype(np.float64), rec[..., 0:3])
    if precision == abi.F64_STRICT:                                 # (every quotient an IEEE division: numpy's)
        assert np.array_equal(rec[..., 0:3] / n[..., None], lin)    # the sum BEFORE its division


def test_a_state_of_another_render_is_refused(scenes, fresh):
    """On a committed scene: another seed, another camera position and another precision each name the field; the scene renders afterwards."""
    ref = fresh(CASE1, abi.F64_STRICT)
    sc, cam, p = _setup(scenes, CASE1, abi.F64_STRICT)
    kw = dict(pass_spp=CASE1["B"], rel_error=CASE1["rel"], abs_error=CASE1["ab"])
    p.seed += 1
    with pytest.raises(abi.RttnwError, match="seed"):
        render.render_adaptive_resume(sc, cam, p, ref[5], **kw)
    p.seed -= 1
    cam.lookfrom[0] += 0.5
    with pytest.raises(abi.RttnwError, match="lookfrom"):
        render.render_adaptive_resume(sc, cam, p, ref[5], **kw)
    cam.lookfrom[0] -= 0.5
    p.precision = abi.F64
    with pytest.raises(abi.RttnwError, match="precision"):
        render.render_adaptive_resume(sc, cam, p, ref[5], **kw)
    p.precision = abi.F64_STRICT
    with pytest.raises(abi.RttnwError, match="no such device"):
        render.render_adaptive_resume(sc, cam, p, ref[5], [0, -1], **kw)
    same_outputs(render.render_adaptive_resume(sc, cam, p, None, **kw), ref, what="afterwards")


def test_state_in_and_state_out_may_be_one_array(gpu, scenes, fresh):
    import ctypes as C
    ref = fresh(CASE1, abi.F64)
    part = fresh(CASE1, abi.F64, cap=48)
    sc, cam, p = _setup(scenes, CASE1, abi.F64)
    a = abi.Adaptive(pass_spp=CASE1["B"], reserved0=0, rel_error=CASE1["rel"], abs_error=CASE1["ab"])
    state = part[5].copy()
    spp = np.zeros((CASE1["h"], CASE1["w"]), dtype=np.uint32)
    rc = gpu.render_adaptive_resume(sc.handle, C.byref(cam), C.byref(p), C.byref(a), 0, None, state.ctypes.data, state.ctypes.data, None, None,
                                    spp.ctypes.data, None, None)
    assert rc == 0, gpu.last_error()
    assert np.array_equal(state, ref[5]) and np.array_equal(spp, ref[2])


def test_cli_round_trip(gpu, tmp_path):
    """--save-state at a cap of 48, --resume to 128: the PNG of the one-shot --spp 128 run, byte for byte."""
    base = [sys.executable, "-m", "rttnw_amd", "7", "--width", "40", "--noise", "0.1", "--pass-spp", "16"]
    a, b, one, state = (str(tmp_path / n) for n in ("a.png", "b.png", "one.png", "a.npy"))
    for argv in (["--spp", "48", "--save-state", state, "--out", a], ["--resume", state, "--spp", "128", "--out", b], ["--spp", "128", "--out", one]):
        r = subprocess.run(base + argv, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert "samples traced of" in r.stdout
    assert np.load(state).shape == (64 + 12 * 40 * 40,)
    assert open(b, "rb").read() == open(one, "rb").read()
    assert open(a, "rb").read() != open(one, "rb").read()
