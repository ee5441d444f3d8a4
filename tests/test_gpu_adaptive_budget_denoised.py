"""rttnw_render_adaptive_budget_denoised on the MI355X, held to its contract (include/rttnw_hip.h): the seven maps, out_valid, state_out, the rounds
and the samples traced are, bit for bit, those of the host composition the header states — the features of rttnw_render_features once, then per
round rttnw_reconstruct on the raw maps so far, the selection restated in numpy (tests/budget_ref.py) on the filtered image and the root of its
variance, and per occupied level rttnw_render_adaptive_region over the mask of that round's pixels at that level, under a cap of (k+1)B and
tolerances of 0 — for every precision, spp_chunk and launch split.  The composition is built HERE, from entry points that existed before this one;
the entry point under test never feeds it.  With 0 iterations the filter is the identity and the call is anchored to rttnw_render_adaptive_budget."""
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
W, H, B, CAP = 48, 40, 16, 128                   # the shapes of tests/test_gpu_adaptive_budget.py
TOL = dict(rel=0.02, ab=0.002)                  # (tighter than that file's 0.05 / 0.01: test_equals_the_composition_bit_for_bit says why)
ROUND_PIXELS = 200
BUDGET = W * H * B + 10 * ROUND_PIXELS * B + 7
ITERATIONS = 3
MAPS = ("linear", "rgba8", "valid", "spp", "stderr", "raw_linear", "raw_stderr")


@pytest.fixture(scope="module")
def scenes(gpu):
    return build_scenes(gpu, ("cornell_box", "final_scene"))


def _setup(scenes, name, precision, spp_chunk=1):
    sc, setup = scenes[name]
    cam, p = S.params_for(setup, W, H, CAP, precision=precision, spp_chunk=spp_chunk)
    return sc, cam, p


def _call(sc, cam, p, samples, round_pixels, rel=TOL["rel"], ab=TOL["ab"], iterations=ITERATIONS, state=None):
    out = render.render_adaptive_budget_denoised(sc, cam, p, samples, round_pixels, state=state, pass_spp=B, rel_error=rel, abs_error=ab,
                                                 iterations=iterations)
    out["samples"] = out["stats"].samples
    return out


def _features(sc, cam, p):
    pf = copy.copy(p)
    pf.spp = B
    return render.render_features(sc, cam, pf)


def rank(raw, features, cap, rel, ab, iterations):
    """Steps 2 and 3 of a round up to the selection's inputs: rttnw_reconstruct on the raw maps, se_f, the own-zero pixels and spp'."""
    den, rgba, var_f, valid = render.reconstruct(raw["raw_linear"], raw["spp"] > 0, features, stderr=raw["raw_stderr"], iterations=iterations)
    se_f = np.sqrt(var_f)
    own_zero = (raw["spp"] > 0) & (raw["raw_stderr"] == 0.0).all(axis=2)
    spp_ranked = np.where(own_zero, np.uint32(cap), raw["spp"]).astype(np.uint32)
    return dict(linear=den, rgba8=rgba, valid=valid, stderr=se_f), own_zero, spp_ranked


def compose(sc, cam, p, samples, round_pixels, rel=TOL["rel"], ab=TOL["ab"], iterations=ITERATIONS):
    """The header's normative composition from no samples, on the host.  A level's call runs under a cap of (k+1)B, and that entry point refuses a
    state with a record above its cap: the records of pixels that stand higher are set aside for the call — they are not selected, so it would
    leave them alone — and put back behind it.  The log holds, per round, what the non-vacuity checks read."""
    h, w, cap = p.height, p.width, p.spp
    features = _features(sc, cam, p)
    raw = dict(raw_linear=np.zeros((h, w, 3)), raw_stderr=np.zeros((h, w, 3)), spp=np.zeros((h, w), np.uint32))
    state, remaining, log = None, int(samples), []
    per_round = round_pixels or -(-w * h // 2)
    while True:
        filtered, own_zero, spp_ranked = rank(raw, features, cap, rel, ab, iterations)
        with np.errstate(all="ignore"):
            mask, rho, m = budget_ref.select(filtered["linear"], filtered["stderr"], spp_ranked, cap, rel, ab, min(per_round, remaining // B))
            # what the own-zero rule keeps out although its filtered error stands above the tolerance
            leaked = int((own_zero & (budget_ref.priority(filtered["linear"], filtered["stderr"], raw["spp"], cap, rel, ab) > 0.0)).sum())
        if m == 0:
            break
        with np.errstate(all="ignore"):
            raw_mask, _, raw_m = budget_ref.select(raw["raw_linear"], raw["raw_stderr"], raw["spp"], cap, rel, ab, m)
        levels = raw["spp"] // B
        occupied = [int(k) for k in np.unique(levels[mask == 1])]
        log.append(dict(m=m, levels=occupied, all_inf=bool(np.isinf(rho[mask == 1]).all()), unsampled_before=int((raw["spp"] == 0).sum()),
                        differs_from_raw=int((raw_mask != mask).sum()), own_zero_above_tolerance=leaked))
        for k in occupied:
            chosen = (mask == 1) & (levels == k)
            pk = copy.copy(p)
            pk.spp = (k + 1) * B
            given = state
            if state is not None:
                given = state.copy()
                aside = (given[64:].reshape(h, w, 12)[..., 3] > pk.spp)
                given[64:].reshape(h, w, 12)[aside] = 0.0
            lin, _, spp, se, _, new = render.render_adaptive_region(sc, cam, pk, 0, 0, w, h, mask=chosen, state=given, device_ids=None, pass_spp=B,
                                                                    rel_error=0.0, abs_error=0.0)
            assert (spp[chosen] == (k + 1) * B).all()
            if state is not None:
                new[64:].reshape(h, w, 12)[aside] = state[64:].reshape(h, w, 12)[aside]
                assert np.array_equal(new[64:].reshape(h, w, 12)[~chosen], state[64:].reshape(h, w, 12)[~chosen])      # nobody else was touched
            state = new
            for key, val in (("raw_linear", lin), ("spp", spp), ("raw_stderr", se)):
                raw[key][chosen] = val[chosen]
        remaining -= m * B
    out = dict(filtered, **raw)
    out.update(state=state, rounds=len(log), samples=int(samples) - remaining, log=log, features=features)
    return out


def _same(got, ref, what="", keys=MAPS):
    for key in keys:
        assert np.array_equal(got[key], ref[key], equal_nan=key in ("stderr", "raw_stderr")), (what, key, int((got[key] != ref[key]).sum()))
    assert np.array_equal(got["state"], ref["state"]), (what, "state")


@pytest.fixture(scope="module")
def guided(scenes):
    """The entry point under test per (scene, spp_chunk, precision) under TOL, BUDGET, ROUND_PIXELS and ITERATIONS, default launch split: computed
    once, shared."""
    cache = {}

    def get(name, spp_chunk, precision):
        key = (name, spp_chunk, precision)
        if key not in cache:
            assert "RTTNW_CHUNK_SUM_BUDGET" not in os.environ
            sc, cam, p = _setup(scenes, name, precision, spp_chunk=spp_chunk)
            cache[key] = _call(sc, cam, p, BUDGET, ROUND_PIXELS)
            for a in cache[key].values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        return cache[key]
    return get


CASES = [(name, 1, precision) for name in ("cornell_box", "final_scene") for precision in PRECISIONS] + [("cornell_box", 0, abi.F64)]


@pytest.mark.parametrize("name,spp_chunk,precision", CASES, ids=["%s-chunk%d-%s" % (n, c, {abi.F64: "f64", abi.F32: "f32", abi.F64_STRICT: "f64strict"}[q])
                                                                  for n, c, q in CASES])
def test_equals_the_composition_bit_for_bit(scenes, guided, name, spp_chunk, precision):
    """48x40, B 16, cap 128, rel_error 0.02, abs_error 0.002, rounds of 200 pixels, a budget of 1920 * 16 + 10 * 200 * 16 + 7 = 62 727 samples, 3
    iterations, default sigmas: the seven maps, out_valid, state_out, the rounds and the samples traced equal the composition's.  Not vacuously —
    the COMPOSITION alone shows that round 0 cuts the +inf group, that at least three rounds run after every pixel holds samples, that a round's
    selection spans two levels, that the final samples map holds at least three values, that the budget is spent to the last whole pass, and that
    in a round after full coverage the selection differs from the one the RAW maps give for the same m (an implementation that ranks by the raw
    error does not pass).
    What was changed from the shapes of tests/test_gpu_adaptive_budget.py: the tolerances, 0.05 / 0.01 there.  Under them the composition on
    cornell_box runs out of candidates — after 16 samples the filter brings all but ~190 pixels below the tolerance, 1244 see black and are kept out
    by the own-zero rule —: 19 rounds that shrink to 2 and 3 pixels and 45 440 (f32: 45 248) of the 62 720 samples, so the budget never bound
    (final_scene spent it).  Under 0.02 / 0.002 every case runs 20 rounds — nine of 200 pixels at level 0, one of 120 + 80 over levels 0 and 1,
    nine of 200 over up to seven levels at once and a last of 120 — and spends the budget down to the 7 left over.  The composition's histogram,
    on an MI355X, of n_q (pixels per sample count; spp_chunk 1 and 0 alike — the Python drivers take 0 as max(1, B / 16) = 1):
      cornell_box  f64 and f64strict  {16: 1511, 32: 56, 48: 40, 64: 36, 80: 36, 96: 27, 112: 21, 128: 193}
                   f32                {16: 1510, 32: 57, 48: 37, 64: 42, 80: 36, 96: 25, 112: 17, 128: 196}
      final_scene  f64 and f64strict  {16: 1550, 32: 32, 48: 17, 64: 43, 80: 28, 96: 22, 112: 13, 128: 215}
                   f32                {16: 1550, 32: 28, 48: 22, 64: 46, 80: 23, 96: 23, 112: 13, 128: 215}
    From round 10 on the selection differs from the raw ranking's in 120 - 390 of the 400 bytes the two set.  The own-zero rule is not idle either: on
    cornell_box up to 597 pixels of a round have a standard error of 0 of their own (they see black, or the light, which emits a constant)
    and a filtered error above the tolerance — their neighbours' noise leaks in —, which is asserted."""
    sc, cam, p = _setup(scenes, name, precision, spp_chunk=spp_chunk)
    ref = compose(sc, cam, p, BUDGET, ROUND_PIXELS)
    log = ref["log"]
    leaked = max(r["own_zero_above_tolerance"] for r in log)
    print("%s spp_chunk %d precision %d: composition ran %d rounds %s, n_q histogram %s, selections that differ from the raw ranking's (pixels per "
          "round) %s, own-zero pixels above the filtered tolerance (most in a round) %d"
          % (name, spp_chunk, precision, ref["rounds"], [(r["m"], r["levels"]) for r in log], _histogram(ref["spp"]),
             [r["differs_from_raw"] for r in log], leaked))
    assert log[0]["m"] == ROUND_PIXELS < W * H and log[0]["all_inf"] and log[0]["levels"] == [0]
    assert sum(1 for r in log if r["unsampled_before"] == 0) >= 3
    assert any(len(r["levels"]) >= 2 for r in log)
    assert len(np.unique(ref["spp"])) >= 3
    assert ref["samples"] == BUDGET - 7
    assert any(r["unsampled_before"] == 0 and r["differs_from_raw"] > 0 for r in log)
    assert name != "cornell_box" or leaked > 0
    got = guided(name, spp_chunk, precision)
    _same(got, ref, name)
    assert got["rounds"] == ref["rounds"]
    assert got["samples"] == ref["samples"] == int(got["spp"].sum(dtype=np.uint64)) and got["stats"].kernel_ms > 0.0
    assert (got["rgba8"][..., 3] == 255 * got["valid"]).all() and np.isinf(got["stderr"][got["valid"] == 0]).all()


@pytest.mark.parametrize("precision", PRECISIONS, ids=["f64", "f32", "f64strict"])
def test_zero_iterations_is_the_budgeted_render(scenes, precision):
    """iterations = 0: the filter is the identity and sqrt(se * se) == se, so the state, out_spp, the raw maps, the rounds and the samples are
    rttnw_render_adaptive_budget's under the same arguments, and out_linear_rgb is the raw image."""
    sc, cam, p = _setup(scenes, "cornell_box", precision)
    lin, rgba, spp, se, st, state, rounds = render.render_adaptive_budget(sc, cam, p, BUDGET, ROUND_PIXELS, pass_spp=B, rel_error=TOL["rel"],
                                                                          abs_error=TOL["ab"])
    got = _call(sc, cam, p, BUDGET, ROUND_PIXELS, iterations=0)
    assert len(np.unique(spp)) >= 3 and rounds >= 12
    assert np.array_equal(got["state"], state) and np.array_equal(got["spp"], spp)
    assert np.array_equal(got["raw_linear"], lin) and np.array_equal(got["raw_stderr"], se, equal_nan=True)
    assert got["rounds"] == rounds and got["samples"] == st.samples
    assert np.array_equal(got["linear"], got["raw_linear"]) and got["valid"].all()
    assert np.array_equal(got["stderr"], se, equal_nan=True)


@pytest.mark.parametrize("name", ["cornell_box", "final_scene"])
def test_outputs_are_the_filter_of_the_raw_outputs(scenes, guided, name):
    """Any run: rttnw_reconstruct on the call's own raw image, raw standard errors, spp > 0 and the features reproduces out_linear_rgb, out_rgba8,
    out_valid and the variance whose root out_stderr_rgb is, bit for bit."""
    sc, cam, p = _setup(scenes, name, abi.F64)
    got = guided(name, 1, abi.F64)
    filtered, _, _ = rank(got, _features(sc, cam, p), CAP, TOL["rel"], TOL["ab"], ITERATIONS)
    _same(dict(got, **filtered), got, name)


def test_a_budget_that_never_binds_is_the_denoised_adaptive_image(scenes):
    """rel_error 0.5 and a budget of w * h * cap samples: every pixel holds samples, out_valid is all 1, and the image is rttnw_denoise of the raw
    maps."""
    sc, cam, p = _setup(scenes, "cornell_box", abi.F64)
    got = _call(sc, cam, p, W * H * CAP, 0, rel=0.5)
    assert (got["spp"] >= B).all() and got["valid"].all() and got["samples"] < W * H * CAP
    den, rgba, var = render.denoise(got["raw_linear"], _features(sc, cam, p), got["raw_stderr"], iterations=ITERATIONS)
    assert np.array_equal(got["linear"], den) and np.array_equal(got["rgba8"], rgba) and np.array_equal(got["stderr"], np.sqrt(var), equal_nan=True)


@pytest.mark.parametrize("precision", PRECISIONS, ids=["f64", "f32", "f64strict"])
def test_from_a_preview_the_unsampled_pixels_come_first(scenes, precision):
    """state_in = rttnw_render_preview(level 2)'s state_out and a budget of exactly the missing pixels times B: every zero record is filled before
    any lattice pixel is touched, and the lattice pixels' records are unchanged."""
    sc, cam, p = _setup(scenes, "cornell_box", precision)
    pv = render.render_preview(sc, cam, p, 2, pass_spp=B, rel_error=TOL["rel"], abs_error=TOL["ab"])
    on = render.lattice_mask(W, H, 2) != 0
    missing = int((~on).sum())
    assert (pv["spp"][~on] == 0).all() and missing == W * H - 12 * 10
    got = _call(sc, cam, p, missing * B, 0, state=pv["state"])
    assert got["samples"] == missing * B and got["rounds"] == -(-missing // (W * H // 2))
    assert (got["spp"][~on] == B).all() and np.array_equal(got["spp"][on], pv["spp"][on])
    before, after = pv["state"][64:].reshape(H, W, 12), got["state"][64:].reshape(H, W, 12)
    assert np.array_equal(after[on], before[on]) and (after[~on][:, 3] == B).all()
    assert np.array_equal(got["raw_linear"][on], pv["raw_linear"][on]) and np.array_equal(got["raw_stderr"][on], pv["raw_stderr"][on], equal_nan=True)


def test_state_in_and_state_out_may_be_the_same_array(scenes):
    sc, cam, p = _setup(scenes, "cornell_box", abi.F64)
    first = _call(sc, cam, p, W * H * B + 500 * B, ROUND_PIXELS)
    want = _call(sc, cam, p, 40 * ROUND_PIXELS * B, ROUND_PIXELS, state=first["state"])
    assert want["samples"] > 0 and not np.array_equal(want["state"], first["state"])
    b = library.product()
    pp = copy.copy(p)
    pp.spp_chunk = max(1, B // 16)
    a = abi.Adaptive(pass_spp=B, reserved0=0, rel_error=TOL["rel"], abs_error=TOL["ab"])
    bg = abi.Budget(samples=40 * ROUND_PIXELS * B, round_pixels=ROUND_PIXELS, reserved0=0)
    g = abi.Guided(feature_spp=0, reserved0=0, denoise=abi.Denoise(iterations=ITERATIONS, reserved0=0, sigma_luminance=0.0, sigma_normal=0.0, sigma_depth=0.0))
    state = first["state"].copy()
    spp = np.zeros((H, W), np.uint32)
    lin = np.zeros((H, W, 3))
    st = abi.Stats()
    rc = b.render_adaptive_budget_denoised(sc.handle, C.byref(cam), C.byref(pp), C.byref(a), C.byref(bg), C.byref(g), state.ctypes.data,
                                           state.ctypes.data, lin.ctypes.data, None, None, spp.ctypes.data, None, None, None, C.byref(st))
    abi.check(rc, b, "rttnw_render_adaptive_budget_denoised")
    assert np.array_equal(state, want["state"]) and np.array_equal(spp, want["spp"]) and np.array_equal(lin, want["linear"])
    assert st.samples == want["samples"]


def test_a_budget_below_one_pass_is_no_work(gpu, scenes):
    """b->samples = 15 < B: RTTNW_OK, nothing traced, no round, and the outputs are the filter of the incoming state — of no state,
    rttnw_reconstruct of nothing: only the background of the pixels whose alpha is 0 (two_spheres: its camera sees the sky beside the spheres)."""
    sc, setup = S.build(gpu, library.scenes(), "two_spheres")
    cam, p = S.params_for(setup, W, H, CAP, precision=abi.F64, spp_chunk=1)
    got = _call(sc, cam, p, 15, ROUND_PIXELS)
    assert got["samples"] == 0 and got["rounds"] == 0
    assert not got["raw_linear"].any() and not got["raw_stderr"].any() and not got["spp"].any() and not got["state"][64:].any()
    features = _features(sc, cam, p)
    filtered, _, _ = rank(got, features, CAP, TOL["rel"], TOL["ab"], ITERATIONS)
    _same(dict(got, **filtered), got, "no state")
    sky = features["alpha"] == 0.0
    print("two_spheres: %d of %d pixels see only the background" % (int(sky.sum()), W * H))
    assert sky.any() and not sky.all()
    assert np.array_equal(got["valid"] != 0, sky) and np.array_equal(got["linear"][sky], features["albedo"][sky]) and not got["linear"][~sky].any()
    assert np.isinf(got["stderr"][~sky]).all()
    # ... and on a state: the outputs of the call that left it
    sc, cam, p = _setup(scenes, "cornell_box", abi.F64)
    first = _call(sc, cam, p, W * H * B + 500 * B, ROUND_PIXELS)
    again = _call(sc, cam, p, 15, ROUND_PIXELS, state=first["state"])
    assert first["samples"] > 0 and again["samples"] == 0 and again["rounds"] == 0
    _same(again, first, "no work on a state")


SPLIT_SCRIPT = """
import sys
import numpy as np
sys.path.insert(0, %r)
from rttnw_amd import abi, library, render
from rttnw_amd import scene as S
b = library.product()
sc, setup = S.build(b, library.scenes(), "cornell_box")
cam, p = S.params_for(setup, %d, %d, %d, precision=abi.F32, spp_chunk=1)
g = render.render_adaptive_budget_denoised(sc, cam, p, %d, %d, pass_spp=%d, rel_error=%r, abs_error=%r, iterations=%d)
np.savez(sys.argv[1], samples=g.pop("stats").samples, **g)
"""


def test_the_launch_split_changes_nothing(guided, tmp_path):
    """A fresh process under RTTNW_CHUNK_SUM_BUDGET=1 — one chunk per launch, sixteen launches per list pass instead of one — gives the same bits."""
    ref = guided("cornell_box", 1, abi.F32)
    out = tmp_path / "split.npz"
    script = SPLIT_SCRIPT % (ROOT, W, H, CAP, BUDGET, ROUND_PIXELS, B, TOL["rel"], TOL["ab"], ITERATIONS)
    r = subprocess.run([sys.executable, "-c", script, str(out)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, RTTNW_CHUNK_SUM_BUDGET="1"))
    assert r.returncode == 0, r.stderr
    got = np.load(out)
    _same(got, ref, "split")
    assert int(got["rounds"]) == ref["rounds"] and int(got["samples"]) == ref["samples"]


def test_cli_guided_budget(gpu, tmp_path):
    """python -m rttnw_amd 7 --noise 0.05 --guided-budget N in a fresh process: both PNGs, the state, the samples traced and the rounds run."""
    from PIL import Image
    r = subprocess.run([sys.executable, "-m", "rttnw_amd", "7", "--width", "96", "--spp", "64", "--pass-spp", "16", "--noise", "0.05", "--guided-budget",
                        "300007", "--spp-map", "m.png", "--save-state", "s.npy"], cwd=tmp_path, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))
    assert r.returncode == 0, r.stderr
    assert Image.open(tmp_path / "image.png").size == (96, 96) and Image.open(tmp_path / "m.png").size == (96, 96)
    assert np.load(tmp_path / "s.npy").size == 64 + 12 * 96 * 96
    assert "guided budget: " in r.stdout and " of 300007 samples in " in r.stdout and "rounds" in r.stdout, r.stdout
