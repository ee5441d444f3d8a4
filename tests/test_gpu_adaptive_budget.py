"""rttnw_render_adaptive_budget on the MI355X, held to its contract (include/rttnw_hip.h): the four outputs, state_out, the rounds and the samples
traced are, bit for bit, those of the host composition the header states — per round the selection restated in numpy (tests/budget_ref.py) on
the maps so far, then per occupied level rttnw_render_adaptive_region over the mask of that round's pixels at that level, under a cap of
(k+1)B and tolerances of 0 — for every precision, spp_chunk and launch split.  The composition is built HERE, from an entry point that existed
before this one; the entry point under test never feeds it."""
import copy
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import budget_ref
from gpu_cases import build_scenes
from gpu_cases import hist as _histogram
from rttnw_amd import abi, library, render
from rttnw_amd import scene as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = [abi.F64, abi.F32, abi.F64_STRICT]
W, H, B, CAP = 48, 40, 16, 128
TOL = dict(rel=0.05, ab=0.01)                    # those of tests/test_gpu_adaptive_denoised.py
ROUND_PIXELS = 200
BUDGET = W * H * B + 10 * ROUND_PIXELS * B + 7
MAPS = ("linear", "rgba8", "spp", "stderr")


@pytest.fixture(scope="module")
def scenes(gpu):
    return build_scenes(gpu, ("cornell_box", "final_scene"))


def _setup(scenes, name, precision, spp_chunk=1):
    sc, setup = scenes[name]
    cam, p = S.params_for(setup, W, H, CAP, precision=precision, spp_chunk=spp_chunk)
    return sc, cam, p


def _budgeted(sc, cam, p, samples, round_pixels, rel=TOL["rel"], ab=TOL["ab"], state=None):
    lin, rgba, spp, se, st, state, rounds = render.render_adaptive_budget(sc, cam, p, samples, round_pixels, state=state, pass_spp=B, rel_error=rel,
                                                                          abs_error=ab)
    return dict(linear=lin, rgba8=rgba, spp=spp, stderr=se, state=state, rounds=rounds, samples=st.samples, stats=st)


def compose(sc, cam, p, samples, round_pixels, rel=TOL["rel"], ab=TOL["ab"]):
    """The header's normative composition from no samples, on the host: numpy's selection and rttnw_render_adaptive_region.  A level's call runs
    under a cap of (k+1)B, and that entry point refuses a state with a record above its cap: the records of pixels that stand higher are set
    aside for the call — they are not selected, so it would leave them alone — and put back behind it."""
    h, w, cap = p.height, p.width, p.spp
    out = dict(linear=np.zeros((h, w, 3)), rgba8=np.zeros((h, w, 4), np.uint8), spp=np.zeros((h, w), np.uint32), stderr=np.zeros((h, w, 3)))
    state, remaining, log = None, int(samples), []
    per_round = round_pixels or -(-w * h // 2)
    while True:
        mask, rho, m = budget_ref.select(out["linear"], out["stderr"], out["spp"], cap, rel, ab, min(per_round, remaining // B))
        if m == 0:
            break
        levels = out["spp"] // B
        occupied = [int(k) for k in np.unique(levels[mask == 1])]
        log.append(dict(m=m, levels=occupied, all_inf=bool(np.isinf(rho[mask == 1]).all()), unsampled_before=int((out["spp"] == 0).sum())))
        for k in occupied:
            chosen = (mask == 1) & (levels == k)
            pk = copy.copy(p)
            pk.spp = (k + 1) * B
            given = state
            if state is not None:
                given = state.copy()
                aside = (given[64:].reshape(h, w, 12)[..., 3] > pk.spp)
                given[64:].reshape(h, w, 12)[aside] = 0.0
            lin, rgba, spp, se, _, new = render.render_adaptive_region(sc, cam, pk, 0, 0, w, h, mask=chosen, state=given, device_ids=None, pass_spp=B,
                                                                       rel_error=0.0, abs_error=0.0)
            assert (spp[chosen] == (k + 1) * B).all()
            if state is not None:
                new[64:].reshape(h, w, 12)[aside] = state[64:].reshape(h, w, 12)[aside]
                assert np.array_equal(new[64:].reshape(h, w, 12)[~chosen], state[64:].reshape(h, w, 12)[~chosen])      # nobody else was touched
            state = new
            for key, val in (("linear", lin), ("rgba8", rgba), ("spp", spp), ("stderr", se)):
                out[key][chosen] = val[chosen]
        remaining -= m * B
    out.update(state=state, rounds=len(log), samples=int(samples) - remaining, log=log)
    return out


def _same(got, ref, what=""):
    for key in MAPS:
        assert np.array_equal(got[key], ref[key], equal_nan=key == "stderr"), (what, key, int((got[key] != ref[key]).sum()))
    assert np.array_equal(got["state"], ref["state"]), (what, "state")


@pytest.fixture(scope="module")
def budgeted(scenes):
    """The entry point under test per (scene, spp_chunk, precision) under TOL, BUDGET and ROUND_PIXELS, default launch split: computed once, shared."""
    cache = {}

    def get(name, spp_chunk, precision):
        key = (name, spp_chunk, precision)
        if key not in cache:
            assert "RTTNW_CHUNK_SUM_BUDGET" not in os.environ
            sc, cam, p = _setup(scenes, name, precision, spp_chunk=spp_chunk)
            cache[key] = _budgeted(sc, cam, p, BUDGET, ROUND_PIXELS)
            for a in cache[key].values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        return cache[key]
    return get


@pytest.mark.parametrize("precision", PRECISIONS, ids=["f64", "f32", "f64strict"])
@pytest.mark.parametrize("spp_chunk", [1, 0])
@pytest.mark.parametrize("name", ["cornell_box", "final_scene"])
def test_equals_the_composition_bit_for_bit(scenes, budgeted, name, spp_chunk, precision):
    """48x40, B 16, cap 128, rel_error 0.05, abs_error 0.01, rounds of 200 pixels, a budget of 1920 * 16 + 10 * 200 * 16 + 7 = 62 727 samples: the
    four outputs, state_out, the rounds and the samples traced equal the composition's.  Not vacuously — the COMPOSITION alone shows that round 0
    cuts the +inf group, that at least three rounds run after every pixel holds samples, that a round's selection spans two levels, that the final
    samples map holds at least three values and that the budget is spent to the last whole pass.
    The composition runs 20 rounds in every case — nine of 200 pixels at level 0, one of 120 + 80 over levels 0 and 1, nine of 200 and a last of
    120 (the 7 samples left over pay for nothing), from round 10 on over up to seven levels at once — and its histogram, on an MI355X, of n_q (pixels per
    sample count; spp_chunk 1 and 0 alike — the Python drivers take 0 as max(1, B / 16) = 1) is:
      cornell_box  f64 and f64strict  {16: 1558, 32: 36, 48: 30, 64: 17, 80: 14, 96: 16, 112: 26, 128: 223}
                   f32                {16: 1559, 32: 34, 48: 30, 64: 18, 80: 15, 96: 15, 112: 26, 128: 223}
      final_scene  f64 and f64strict  {16: 1448, 32: 33, 48: 37, 64: 59, 80: 126, 96: 117, 112: 73, 128: 27}
                   f32                {16: 1446, 32: 32, 48: 41, 64: 58, 80: 128, 96: 116, 112: 73, 128: 26}"""
    sc, cam, p = _setup(scenes, name, precision, spp_chunk=spp_chunk)
    ref = compose(sc, cam, p, BUDGET, ROUND_PIXELS)
    log = ref["log"]
    print("%s spp_chunk %d precision %d: composition ran %d rounds %s, n_q histogram %s"
          % (name, spp_chunk, precision, ref["rounds"], [(r["m"], r["levels"]) for r in log], _histogram(ref["spp"])))
    assert log[0]["m"] == ROUND_PIXELS < W * H and log[0]["all_inf"] and log[0]["levels"] == [0]
    assert sum(1 for r in log if r["unsampled_before"] == 0) >= 3
    assert any(len(r["levels"]) >= 2 for r in log)
    assert len(np.unique(ref["spp"])) >= 3
    assert ref["samples"] == BUDGET - 7
    got = budgeted(name, spp_chunk, precision)
    _same(got, ref, name)
    assert got["rounds"] == ref["rounds"]
    assert got["samples"] == ref["samples"] == int(got["spp"].sum(dtype=np.uint64)) and got["stats"].kernel_ms > 0.0


@pytest.mark.parametrize("precision", PRECISIONS, ids=["f64", "f32", "f64strict"])
def test_a_budget_that_never_binds_is_the_resumed_render(scenes, precision):
    """rel_error 0.5 and a budget of w * h * cap samples: the outputs and the state of rttnw_render_adaptive_resume(state = None) under the same
    cap, B and tolerances, bit for bit, whatever the size of a round — half the frame, one pixel, 333 pixels."""
    sc, cam, p = _setup(scenes, "cornell_box", precision)
    lin, rgba, spp, se, st, state = render.render_adaptive_resume(sc, cam, p, None, None, pass_spp=B, rel_error=0.5, abs_error=TOL["ab"])
    ref = dict(linear=lin, rgba8=rgba, spp=spp, stderr=se, state=state)
    assert len(np.unique(spp)) >= 2 and (spp < CAP).any()
    rounds = {}
    for round_pixels in (0, 1, 333):
        got = _budgeted(sc, cam, p, W * H * CAP, round_pixels, rel=0.5)
        _same(got, ref, round_pixels)
        assert got["samples"] == st.samples == int(spp.sum(dtype=np.uint64))
        rounds[round_pixels] = got["rounds"]
    print("precision %d: rounds %s, n_q histogram %s" % (precision, rounds, _histogram(spp)))
    assert rounds[1] == st.samples // B and rounds[0] < rounds[333] < rounds[1]


@pytest.mark.parametrize("precision", [abi.F64, abi.F32], ids=["f64", "f32"])
def test_its_state_resumes_over_three_ranks_with_nothing_left_to_do(scenes, precision):
    """The two host paths of a state, crossed: state_out of the one-rank form (the whole frame in one packed order) goes in as state_in of
    rttnw_render_adaptive_resume over device_ids [0, 0, 0] (three ranks' packed orders), under the same cap, B and tolerances.  cornell_box 45x37 —
    edge tiles on both axes, 30 tiles over 3 ranks —, cap 32, B 8, a budget of w * h * cap samples, which never binds: every pixel has stopped or
    stands at the cap, so the resumed call traces nothing, hands the state back bit for bit and reports the budget call's four outputs."""
    w, h, cap, b = 45, 37, 32, 8
    sc, setup = scenes["cornell_box"]
    cam, p = S.params_for(setup, w, h, cap, precision=precision, spp_chunk=1)
    lin, rgba, spp, se, st, state, rounds = render.render_adaptive_budget(sc, cam, p, w * h * cap, 0, pass_spp=b, rel_error=0.5, abs_error=TOL["ab"])
    print("precision %d: %d rounds, n_q histogram %s" % (precision, rounds, _histogram(spp)))
    assert state.shape == (64 + 12 * w * h,) and (spp >= b).all() and st.samples == int(spp.sum(dtype=np.uint64))
    given = state.copy()
    lin_r, rgba_r, spp_r, se_r, st_r, state_r = render.render_adaptive_resume(sc, cam, p, given, [0, 0, 0], pass_spp=b, rel_error=0.5,
                                                                              abs_error=TOL["ab"])
    assert np.array_equal(given, state)                                        # state_in is read only
    assert np.array_equal(state_r.view(np.uint64), state.view(np.uint64))
    assert sum(s.samples for s in st_r) == 0
    for key, got, ref in (("linear", lin_r, lin), ("rgba8", rgba_r, rgba), ("spp", spp_r, spp), ("stderr", se_r, se)):
        assert np.array_equal(got, ref, equal_nan=key == "stderr"), (key, int((got != ref).sum()))


@pytest.mark.parametrize("precision", PRECISIONS, ids=["f64", "f32", "f64strict"])
def test_from_a_preview_the_unsampled_pixels_come_first(scenes, precision):
    """state_in = rttnw_render_preview(level 2)'s state_out and a budget of exactly the missing pixels times B: every zero record is filled before
    any other pixel is touched, and the lattice pixels' records are unchanged."""
    sc, cam, p = _setup(scenes, "cornell_box", precision)
    pv = render.render_preview(sc, cam, p, 2, pass_spp=B, rel_error=TOL["rel"], abs_error=TOL["ab"])
    on = render.lattice_mask(W, H, 2) != 0
    missing = int((~on).sum())
    assert (pv["spp"][~on] == 0).all() and missing == W * H - 12 * 10
    got = _budgeted(sc, cam, p, missing * B, 0, state=pv["state"])
    assert got["samples"] == missing * B and got["rounds"] == -(-missing // (W * H // 2))
    assert (got["spp"][~on] == B).all() and np.array_equal(got["spp"][on], pv["spp"][on])
    before, after = pv["state"][64:].reshape(H, W, 12), got["state"][64:].reshape(H, W, 12)
    assert np.array_equal(after[on], before[on]) and (after[~on][:, 3] == B).all()
    assert np.array_equal(got["linear"][on], pv["raw_linear"][on]) and np.array_equal(got["stderr"][on], pv["raw_stderr"][on], equal_nan=True)
    # ... and the filled pixels are the fresh adaptive render's first pass, bit for bit
    p1 = copy.copy(p)
    p1.spp = B
    lin, _, _, se, _, _ = render.render_adaptive_resume(sc, cam, p1, None, None, pass_spp=B, rel_error=0.0, abs_error=0.0)
    assert np.array_equal(got["linear"][~on], lin[~on]) and np.array_equal(got["stderr"][~on], se[~on], equal_nan=True)


def test_state_in_and_state_out_may_be_the_same_array(scenes):
    sc, cam, p = _setup(scenes, "cornell_box", abi.F64)
    first = _budgeted(sc, cam, p, W * H * B + 500 * B, ROUND_PIXELS)
    want = _budgeted(sc, cam, p, 40 * ROUND_PIXELS * B, ROUND_PIXELS, state=first["state"])
    assert want["samples"] > 0 and not np.array_equal(want["state"], first["state"])
    b = library.product()
    pp = copy.copy(p)
    pp.spp_chunk = max(1, B // 16)
    a = abi.Adaptive(pass_spp=B, reserved0=0, rel_error=TOL["rel"], abs_error=TOL["ab"])
    g = abi.Budget(samples=40 * ROUND_PIXELS * B, round_pixels=ROUND_PIXELS, reserved0=0)
    state = first["state"].copy()
    spp = np.zeros((H, W), np.uint32)
    st = abi.Stats()
    rc = b.render_adaptive_budget(sc.handle, C.byref(cam), C.byref(pp), C.byref(a), C.byref(g), state.ctypes.data, state.ctypes.data, None, None,
                                  spp.ctypes.data, None, C.byref(st))
    abi.check(rc, b, "rttnw_render_adaptive_budget")
    assert np.array_equal(state, want["state"]) and np.array_equal(spp, want["spp"]) and st.samples == want["samples"]


def test_a_budget_below_one_pass_is_no_work(scenes):
    """b->samples = 15 < B: RTTNW_OK, nothing traced, no round, the outputs of the incoming state — of no state, zeros, alpha included."""
    sc, cam, p = _setup(scenes, "cornell_box", abi.F64)
    got = _budgeted(sc, cam, p, 15, ROUND_PIXELS)
    assert got["samples"] == 0 and got["rounds"] == 0
    assert not got["linear"].any() and not got["rgba8"].any() and not got["spp"].any() and not got["stderr"].any() and not got["state"][64:].any()
    first = _budgeted(sc, cam, p, W * H * B + 500 * B, ROUND_PIXELS)
    again = _budgeted(sc, cam, p, 15, ROUND_PIXELS, state=first["state"])
    assert again["samples"] == 0 and again["rounds"] == 0
    _same(again, first, "no work on a state")
    # ... and the same when the budget is ample and no candidate is left: every pixel at the cap of this call
    p1 = copy.copy(p)
    p1.spp = B
    full = render.render_adaptive_budget(sc, cam, p1, W * H * B, 0, pass_spp=B, rel_error=TOL["rel"], abs_error=TOL["ab"])
    more = render.render_adaptive_budget(sc, cam, p1, W * H * B, 0, state=full[5], pass_spp=B, rel_error=TOL["rel"], abs_error=TOL["ab"])
    assert full[4].samples == W * H * B and more[4].samples == 0 and more[6] == 0 and np.array_equal(more[5], full[5]) and np.array_equal(more[0], full[0])


def test_levels_beyond_one_sweep_of_the_census(gpu):
    """B = 1 and a state whose pixels hold 260 samples: the rounds run at levels 260 .. 263, beyond the 256 levels the census counts in one
    sweep of its LDS bins.  With an ample budget the call is rttnw_render_adaptive_resume from the same state under the same cap, bit for bit.
    (two_spheres under its sky: no two samples of a pixel are alike, so a tolerance of 0 stops nobody before the cap; rel_error 1e-4 keeps
    nearly every pixel a candidate at 260 samples.)"""
    sc, setup = S.build(gpu, library.scenes(), "two_spheres")
    rel, ab = 1e-4, 0.0
    w, h = 24, 16
    cam, p = S.params_for(setup, w, h, 260, precision=abi.F64, spp_chunk=1)
    start = render.render_adaptive_resume(sc, cam, p, None, None, pass_spp=1, rel_error=0.0, abs_error=0.0)
    assert (start[2] == 260).sum() > 100
    p.spp = 264
    lin, rgba, spp, se, st, state = render.render_adaptive_resume(sc, cam, p, start[5], None, pass_spp=1, rel_error=rel, abs_error=ab)
    assert st.samples > 100 and (spp == 264).sum() > 50                    # the passes at levels 260 .. 263 are not a handful of pixels'
    got = render.render_adaptive_budget(sc, cam, p, w * h * 8, 37, state=start[5], pass_spp=1, rel_error=rel, abs_error=ab)
    assert np.array_equal(got[5], state) and np.array_equal(got[0], lin) and np.array_equal(got[1], rgba) and np.array_equal(got[2], spp)
    assert np.array_equal(got[3], se, equal_nan=True) and got[4].samples == st.samples and got[6] >= 4


SPLIT_SCRIPT = """
import sys
import numpy as np
sys.path.insert(0, %r)
from rttnw_amd import abi, library, render
from rttnw_amd import scene as S
b = library.product()
sc, setup = S.build(b, library.scenes(), "cornell_box")
cam, p = S.params_for(setup, %d, %d, %d, precision=abi.F32, spp_chunk=1)
lin, rgba, spp, se, st, state, rounds = render.render_adaptive_budget(sc, cam, p, %d, %d, pass_spp=%d, rel_error=%r, abs_error=%r)
np.savez(sys.argv[1], linear=lin, rgba8=rgba, spp=spp, stderr=se, state=state, rounds=rounds, samples=st.samples)
"""


def test_the_launch_split_changes_nothing(budgeted, tmp_path):
    """A fresh process under RTTNW_CHUNK_SUM_BUDGET=1 — one chunk per launch, sixteen launches per list pass instead of one — gives the same bits."""
    ref = budgeted("cornell_box", 1, abi.F32)
    out = tmp_path / "split.npz"
    script = SPLIT_SCRIPT % (ROOT, W, H, CAP, BUDGET, ROUND_PIXELS, B, TOL["rel"], TOL["ab"])
    r = subprocess.run([sys.executable, "-c", script, str(out)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, RTTNW_CHUNK_SUM_BUDGET="1"))
    assert r.returncode == 0, r.stderr
    got = np.load(out)
    _same(got, ref, "split")
    assert int(got["rounds"]) == ref["rounds"] and int(got["samples"]) == ref["samples"]


def test_cli_budget(gpu, tmp_path):
    """python -m rttnw_amd 7 --noise 0.05 --budget N in a fresh process: both PNGs, the state, the samples traced and the rounds run."""
    from PIL import Image
    r = subprocess.run([sys.executable, "-m", "rttnw_amd", "7", "--width", "96", "--spp", "64", "--pass-spp", "16", "--noise", "0.05", "--budget", "300007",
                        "--spp-map", "m.png", "--save-state", "s.npy"], cwd=tmp_path, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))
    assert r.returncode == 0, r.stderr
    assert Image.open(tmp_path / "image.png").size == (96, 96) and Image.open(tmp_path / "m.png").size == (96, 96)
    assert np.load(tmp_path / "s.npy").size == 64 + 12 * 96 * 96
    assert "budget: 300000 of 300007 samples in " in r.stdout and "rounds" in r.stdout, r.stdout
