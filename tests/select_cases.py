"""What the tests of rttnw_denoise_select share (tests/test_select_cpu.py on the host harness, tests/test_gpu_select.py on the device): the frames
and parameter sets both are held to, and the checks of the properties both must have.  An implementation under test is a function
run(half_a, half_b, features, var_a=None, var_b=None, **parameters) -> dict of select_ref.OUTPUTS."""
import numpy as np

import denoise_ref
import nlm_ref
import select_ref
from nlm_cases import FRAMES, crop_interior, same_bits

# (s, t): the smallest, the defaults, the largest (the device's LDS at its fullest) and a blend window wider than the error window
RADII = [(1, 1), (5, 2), (16, 8), (3, 8)]
MARGINS = [0.0, 0.01, -0.3]
ITERATIONS = [0, 5]
NLM_RADII = [(1, 1), (0, 0)]  # (0, 0): the defaults, 7 and 3
# the filters' settings a frame is filtered with once, and the selections made from each
FILTER_SETS = [(size, with_variance, iterations, nlm_radii) for size in FRAMES for with_variance in (True, False) for iterations in ITERATIONS
               for nlm_radii in NLM_RADII]
FILTER_IDS = ["%dx%d-%s-it%d-r%d-f%d" % (s[0], s[1], "variance" if v else "pair-variance", it, rf[0], rf[1]) for s, v, it, rf in FILTER_SETS]


def inputs(seed, w, h, with_variance=True):
    """Colour and variances of nlm_ref.random_inputs (finite), features of denoise_ref.random_inputs (alpha 0, short normals, albedo below the
    demodulation threshold): (half_a, half_b, var_a, var_b, features)."""
    rng = np.random.default_rng(seed)
    a, b, va, vb = nlm_ref.random_inputs(rng, w, h, with_variance)
    return a, b, va, vb, denoise_ref.random_inputs(rng, w, h, False)[2]


def filter_set_inputs(case):
    size, with_variance, iterations, nlm_radii = case
    return inputs(size[0] * 64 + iterations * 4 + nlm_radii[0] * 2 + int(with_variance), size[0], size[1], with_variance)


def assert_same_outputs(got, want, what=()):
    for name in select_ref.OUTPUTS:
        assert same_bits(got[name], want[name]), (name,) + tuple(what) + (float(np.nanmax(np.abs(got[name].astype(np.float64) - want[name]))),)


def check_composition(run, denoise, nlm, with_variance):
    """Margin 2 gives beta == 0 and the mean of two `denoise` calls; margin -2 gives beta == 1 and `nlm`'s image: bit for bit.
    denoise(colour, variance, features, iterations) -> linear; nlm(a, b, var_a, var_b) -> the dict of nlm_ref.OUTPUTS."""
    a, b, va, vb, f = inputs(21 + int(with_variance), 37, 29, with_variance)
    if with_variance:   # exact squares, so that a `denoise` that takes standard errors and squares them is handed these very variances
        va, vb = np.square(np.sqrt(va)), np.square(np.sqrt(vb))
    fa, fb = denoise(a, va, f, 3), denoise(b, vb, f, 3)
    only_f = run(a, b, f, va, vb, iterations=3, margin=2.0)
    assert np.all(only_f["blend"] == 0.0)
    assert same_bits(only_f["linear"], (fa + fb) * 0.5) and same_bits(only_f["feature"], only_f["linear"])
    d = fa - fb
    assert same_bits(only_f["error"], (d * d) * 0.25)
    whole = nlm(a, b, va, vb)
    only_n = run(a, b, f, va, vb, iterations=3, margin=-2.0)
    assert np.all(only_n["blend"] == 1.0)
    for name in ("linear", "rgba8", "error"):
        assert same_bits(only_n[name], whole[name]), name
    assert same_bits(only_n["nlm"], whole["linear"]) and same_bits(only_n["feature"], only_f["feature"])
    assert not same_bits(only_n["linear"], only_f["linear"])


def check_unchosen_nan_stays_out(run):
    """A NaN variance makes non-local means' half NaN around it (nlm.hpp: not special-cased) while the feature-guided filter, which drops a
    variance that is not finite, stays finite: d is NaN there, a NaN window sum chooses the feature-guided filter, and — the blend window being
    no wider than the error window at the defaults — beta is exactly 0 wherever non-local means is NaN."""
    a, b, va, vb, f = inputs(5, 40, 33)
    vb = vb.copy()
    vb[16, 20] = np.nan
    out = run(a, b, f, va, vb)
    bad = np.isnan(out["nlm"]).any(axis=-1)
    assert bad[16, 20] and np.isfinite(out["feature"]).all()
    assert np.all(out["blend"][bad] == 0.0)
    assert np.isfinite(out["linear"]).all() and np.isfinite(out["error"]).all()
    assert same_bits(out["linear"][bad], out["feature"][bad])
    assert (out["blend"] > 0.0).any()                                 # ... and elsewhere the choice still goes both ways


def check_exchange(run, with_variance):
    a, b, va, vb, f = inputs(3 + int(with_variance), 37, 29, with_variance)
    one, other = run(a, b, f, va, vb), run(b, a, f, vb, va)
    assert_same_outputs(one, other)
    assert 0.0 < one["blend"].mean() < 1.0                            # both filters were chosen somewhere: the exchange was of something


LOCALITY_ITERATIONS = 2


def locality_margin(error_radius=0, blend_radius=0, search_radius=0, patch_radius=0):
    r, fr = search_radius or nlm_ref.DEFAULTS["search_radius"], patch_radius or nlm_ref.DEFAULTS["patch_radius"]
    s, t = error_radius or select_ref.DEFAULTS["error_radius"], blend_radius or select_ref.DEFAULTS["blend_radius"]
    return max(r + fr + 1, 2 * (2 ** LOCALITY_ITERATIONS - 1)) + s + t


def check_locality(run, a, b, va, vb, f, crop, **kw):
    """The interior of a crop taken with the stated margin equals the same pixels of the whole frame's result, bit for bit."""
    m = locality_margin(**kw)
    whole = run(a, b, f, va, vb, iterations=LOCALITY_ITERATIONS, **kw)
    cut = lambda x: None if x is None else x[crop]
    part = run(a[crop], b[crop], {k: v[crop] for k, v in f.items() if k != "stats"}, cut(va), cut(vb), iterations=LOCALITY_ITERATIONS, **kw)
    assert min(crop_interior(part["linear"], m).shape[:2]) >= 5
    for name in select_ref.OUTPUTS:
        assert same_bits(crop_interior(part[name], m), crop_interior(whole[name][crop], m)), name
    assert not same_bits(part["linear"], whole["linear"][crop])       # ... and the crop's edge is felt somewhere
