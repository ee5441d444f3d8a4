"""The regression stage of the rttnw_svgf handle without a GPU: the host build of the arithmetic the device kernels run (rttnw_amd/csrc/svgf.hpp
and the headers it composes, built by tests/svgf_regress_host) against the contract of include/rttnw_hip.h restated as a composition of the
stages' restatements (tests/svgf_regress_ref.py) — bit for bit, every field of rttnw_svgf_out and of rttnw_svgf_halves, along chains of three
calls — and the consequences the contract states, on both."""
import numpy as np
import pytest

import nlm_ref
import svgf_ref
import svgf_regress_ref as R
from temporal_cases import same

IMPLEMENTATIONS = [R.Restated, R.Host]
IDS = ["restatement", "host-build"]


def test_the_cases_cover_what_they_claim():
    assert {c[0] for c in R.CASES} == {(45, 37), (70, 9), (5, 3)}
    for size in R.SIZES:
        assert {c[1:4] for c in R.CASES if c[0] == size and not c[4] and not c[5]} == {(dm, m, s) for dm in (0, 1) for m in (0, 7) for s in (0, 1)}
    assert sum(1 for c in R.CASES if c[4]) == 5 and sum(1 for c in R.CASES if c[5]) == 1
    for case in R.CASES:
        fr = R.frames(case)
        assert len(fr) == 3 and all((f["alpha"] == 0.0).any() for _, _, f, _ in fr)                  # a region of alpha == 0 in every frame
        assert [bool(np.isnan(a).any()) for a, _, _, _ in fr] == [False, bool(case[4]), False]         # one NaN, in half_a of the second frame
        assert np.isnan(fr[1][0]).sum() == (1 if case[4] else 0)
        assert (fr[0][2]["albedo"] <= svgf_ref.ALBEDO_EPS).any() or case[0] == (5, 3)


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_host_build_equals_the_restatement_bit_for_bit(case):
    R.check_chain(R.Host, R.Restated, case)


@pytest.mark.parametrize("make", IMPLEMENTATIONS, ids=IDS)
def test_a_nan_propagates_and_is_not_special_cased(make):
    """The NaN of the second frame reaches that frame's result and, through Ha, the third frame's; it stays within the filter's reach of its pixel."""
    case = next(c for c in R.CASES if c[4] and c[2] == 7 and c[3] == 0)
    (w, h) = case[0]
    seq = make(w, h, **R.settings(case))
    outs = [seq.push_halves(*fr) for fr in R.frames(case)]
    assert np.isfinite(outs[0]["linear_rgb"]).all()
    for k in (1, 2):
        bad = np.isnan(outs[k]["linear_rgb"]).any(axis=-1)
        assert bad.any() and np.isnan(outs[k]["acc_a"]).any() and not np.isnan(outs[k]["acc_b"]).any(), k
        ys, xs = np.nonzero(bad)
        assert np.abs(ys - h // 2).max() <= 8 and np.abs(xs - w // 2).max() <= 8, k          # r + f + 1 = 4 pixels a frame, and the reprojection's tap


@pytest.mark.parametrize("make", IMPLEMENTATIONS, ids=IDS)
@pytest.mark.parametrize("demodulate", [0, 1])
def test_the_shared_outputs_are_a_plain_handles_pushed_with_the_mean(make, demodulate):
    """The consequence under step 1: M1, M2, length, prev_xy and the estimate do not know about the halves."""
    case = (R.SIZES[0], demodulate, 7, 0, False, False)
    (w, h) = case[0]
    kw = R.settings(case)
    plain = (svgf_ref.Restated if make is R.Restated else svgf_ref.Host)(w, h, feedback=0, demodulate=kw["demodulate"], min_temporal=kw["min_temporal"],
                                                                        radius=kw["radius"], iterations=kw["iterations"])
    seq = make(w, h, **kw)
    for k, (a, b, f, cam) in enumerate(R.frames(case)):
        got, want = seq.push_halves(a, b, f, cam), plain.push((a + b) * 0.5, f, cam)
        for name in ("moment1_rgb", "moment2_rgb", "length", "prev_xy", "variance_rgb", "history_rgb", "raw_rgb", "albedo", "normal", "depth", "alpha"):
            assert same(got[name], want[name]), (name, k)
        assert not same(got["linear_rgb"], want["linear_rgb"]), k                               # ... and the spatial stage is another


@pytest.mark.parametrize("make", IMPLEMENTATIONS, ids=IDS)
@pytest.mark.parametrize("source", [0, 1])
def test_without_features_the_stage_is_non_local_means(make, source):
    """features == 0: step 3 is rttnw_denoise_nlm(Aa, Ab, var + var, var + var) — or over the pair variance — bit for bit, multiplied back."""
    case = (R.SIZES[0], 1, 0, source, False, False)
    (w, h) = case[0]
    seq = make(w, h, **R.settings(case))
    for k, (a, b, f, cam) in enumerate(R.frames(case)):
        got = seq.push_halves(a, b, f, cam)
        v2 = got["variance_rgb"] + got["variance_rgb"] if source == 0 else None
        want = nlm_ref.denoise_nlm(got["acc_a"], got["acc_b"], v2, v2, **R.SMALL_RADII)
        divided = (f["alpha"][..., None] != 0.0) & (f["albedo"] > svgf_ref.ALBEDO_EPS)
        assert same(got["linear_rgb"], np.where(divided, want["linear"] * f["albedo"], want["linear"])), k
        assert same(got["filtered_a"], want["half_a"]) and same(got["filtered_b"], want["half_b"]) and same(got["filtered_variance_rgb"], want["error"]), k
        assert np.array_equal(got["fit"], 2.0 * np.ones((h, w))), k                               # d == 0: the formulas are the zero-order value's


@pytest.mark.parametrize("make", IMPLEMENTATIONS, ids=IDS)
def test_the_halves_accumulate(make):
    """On a static camera with a flat albedo the accumulated halves' noise falls with the frames, and their mean is the accumulation shown."""
    case = (R.SIZES[0], 0, 7, 0, False, False)
    (w, h) = case[0]
    seq = make(w, h, **R.settings(case))
    fr = R.frames(case)
    cam, f = fr[0][3], fr[0][2]
    rng = np.random.default_rng(5)
    spread = []
    for k in range(4):
        a, b = 0.5 + 0.1 * rng.standard_normal((h, w, 3)), 0.5 + 0.1 * rng.standard_normal((h, w, 3))
        got = seq.push_halves(a, b, f, cam)
        hit = f["alpha"] != 0.0
        spread.append(float(np.std(got["acc_a"][hit])))
        assert same(got["accumulated_rgb"], (got["acc_a"] + got["acc_b"]) * 0.5), k
    assert spread[3] < 0.6 * spread[0], spread                                                    # 1 / sqrt(4) = 0.5 of the first frame's
