"""What the tests of rttnw_denoise and rttnw_reconstruct share (tests/test_denoise_cpu.py and tests/test_reconstruct_cpu.py on the host builds,
tests/test_gpu_denoise.py and tests/test_gpu_reconstruct.py on the device): the frame sizes, iteration counts and sigmas both are held to, frames
with every value the header's contract allows and a render never has, the validity masks of reconstruct, the numpy restatement's result of every
case (computed once per process, read-only), and the checks of the properties both must have.  An implementation of rttnw_denoise under test is a
function run(colour, variance or None, features, iterations, **sigmas) -> (linear, rgba8, variance or None)."""
import functools

import numpy as np

import denoise_ref
import reconstruct_ref
from temporal_cases import same

# 33x9: one ragged column and one ragged row beyond the device's 32x8 blocks, n*3 no multiple of its flat 256-thread blocks; 129x7 and 7x129: a
# swapped width and height, and a stride-128 tap (pass 8) inside the image for exactly one column (row); 1x1 and 3x5: smaller than any block
SIZES = [(1, 1), (3, 5), (33, 9), (45, 37), (70, 41), (129, 7), (7, 129)]
ITERATIONS = (0, 1, 2, 5, 8)            # 8 is DENOISE_MAX_ITERATIONS: strides 32, 64 and 128 put almost every tap outside these frames
# the defaults; sigma_normal 1 is 0 squarings of the normal weight, 2000 stops at the cap of 10
SIGMAS = [{}, dict(sigma_luminance=1.5, sigma_normal=1.0, sigma_depth=0.02), dict(sigma_luminance=9.0, sigma_normal=2000.0, sigma_depth=0.5)]
SIGMA_IDS = ["defaults", "0-squarings", "10-squarings"]
FRAMES = [(size, v) for size in SIZES for v in (True, False)]
FRAME_IDS = ["%dx%d-%s" % (s[0], s[1], "variance" if v else "plain") for s, v in FRAMES]
HOSTILE_PERCENT = 4                      # of the pixels, for each of: zero normal, negated depth, zero depth
NON_VACUOUS_FROM = 297                   # pixels (33x9): from here on a frame must hold every kind of value
MASK_IDS = ["random0.02", "random0.3", "random1.0", "lattice2"]


def frame_seed(size, with_variance):
    return 1000 * size[0] + 10 * size[1] + int(with_variance)


def hostile_inputs(seed, w, h, with_variance=True):
    """denoise_ref.random_inputs, and on three disjoint random subsets of HOSTILE_PERCENT of the pixels each: a zero normal (every tap weighs 0), a
    negated depth, a zero depth (with another one beside it the depth weight's denominator is `tiny` alone).  Nothing the contract excludes."""
    rng = np.random.default_rng(seed)
    colour, var, f = denoise_ref.random_inputs(rng, w, h, with_variance)
    n = w * h
    k = (n * HOSTILE_PERCENT + 99) // 100
    order = rng.permutation(n)
    normal, depth = f["normal"].reshape(n, 3), f["depth"].reshape(n)        # views: the frame's own arrays
    normal[order[:k]] = 0.0
    depth[order[k:2 * k]] *= -1.0
    depth[order[2 * k:3 * k]] = 0.0
    return colour, var, f


def kinds(colour, var, f):
    """How many pixels of a frame hold each kind of value the device never saw in a render: counted on the inputs alone."""
    hit = f["alpha"] != 0.0
    counts = {"zero normal": hit & (f["normal"] == 0.0).all(axis=-1), "negative depth": hit & (f["depth"] < 0.0), "zero depth": hit & (f["depth"] == 0.0),
              "alpha 0": ~hit, "fractional alpha": hit & (f["alpha"] < 1.0),
              "albedo in (0, eps]": hit & ((f["albedo"] > 0.0) & (f["albedo"] <= denoise_ref.ALBEDO_EPS)).any(axis=-1),
              "albedo across eps": hit & (f["albedo"] <= denoise_ref.ALBEDO_EPS).any(axis=-1) & (f["albedo"] > denoise_ref.ALBEDO_EPS).any(axis=-1)}
    if var is not None:
        counts.update({"variance inf": hit & np.isinf(var).any(axis=-1), "variance NaN": hit & np.isnan(var).any(axis=-1),
                       "variance 0": hit & (var == 0.0).all(axis=-1)})
    return {k: int(v.sum()) for k, v in counts.items()}


def assert_not_vacuous(size, with_variance):
    counts = kinds(*frame(size, with_variance))
    if size[0] * size[1] >= NON_VACUOUS_FROM:
        assert min(counts.values()) >= 1, (size, with_variance, counts)
    return counts


def _freeze(*arrays):
    for a in arrays:
        if isinstance(a, dict):
            _freeze(*a.values())
        elif a is not None:
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def frame(size, with_variance):
    """(colour, variance or None, features) of a size of SIZES: computed once, read-only."""
    return _freeze(*hostile_inputs(frame_seed(size, with_variance), size[0], size[1], with_variance))


def valid_masks(rng, w, h):
    """(name, HxW bool) of reconstruct's validity patterns: random at three densities — 0.02 leaves most pixels to be filled over several passes and
    some never —, and the preview's lattice at level 2."""
    for density in (0.02, 0.3, 1.0):
        yield "random%s" % density, rng.random((h, w)) < density
    yield "lattice2", reconstruct_ref.lattice(w, h, 2)


def poisoned(colour, var, valid):
    """Colour and variance with NaN wherever `valid` is 0: never read there."""
    c = np.where(valid[..., None], colour, np.nan)
    return c, None if var is None else np.where(valid[..., None], var, np.nan)


@functools.lru_cache(maxsize=None)
def masked_frames(size, with_variance):
    """{mask name: (poisoned colour, poisoned variance or None, valid)} of a frame, read-only."""
    colour, var, _ = frame(size, with_variance)
    rng = np.random.default_rng(frame_seed(size, with_variance) + 500000)
    return {name: _freeze(*poisoned(colour, var, valid), valid) for name, valid in valid_masks(rng, size[0], size[1])}


@functools.lru_cache(maxsize=None)
def denoise_reference(size, with_variance, iterations, sigma):
    """denoise_ref.denoise of a case (`sigma`: an index into SIGMAS), read-only."""
    colour, var, f = frame(size, with_variance)
    return _freeze(*denoise_ref.denoise(colour, var, f, iterations, **SIGMAS[sigma]))


@functools.lru_cache(maxsize=None)
def reconstruct_reference(size, with_variance, mask, iterations, sigma):
    """reconstruct_ref.reconstruct of a case, read-only."""
    c, v, valid = masked_frames(size, with_variance)[mask]
    return _freeze(*reconstruct_ref.reconstruct(c, v, valid, frame(size, with_variance)[2], iterations, **SIGMAS[sigma]))


def assert_same_results(got, want, what=()):
    """Every output of a call, every pixel: the same bits, a NaN standing for any NaN (a variance that passes through arithmetic as a NaN comes
    out with the processor's payload)."""
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert same(a, b), (k,) + tuple(what)


def same_bits(a, b):
    """The same bits, NaNs included: for values that pass through untouched."""
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def fill_counts(size, with_variance, mask, iterations, sigma=0):
    """Of reconstruct_reference's output: (pixels filled from their taps, pixels never filled, filled pixels with no finite-variance tap — their
    variance is +inf).  The background a miss returns (alpha 0) is not counted as filled."""
    valid = masked_frames(size, with_variance)[mask][2]
    hit = frame(size, with_variance)[2]["alpha"] != 0.0
    _, _, out_var, ok = reconstruct_reference(size, with_variance, mask, iterations, sigma)
    filled = (ok != 0) & ~valid & hit
    no_variance = filled & np.isposinf(out_var).all(axis=-1) if out_var is not None else np.zeros_like(filled)
    return int(filled.sum()), int((ok == 0).sum()), int(no_variance.sum())


# ---- properties

def check_zero_iterations_is_the_identity(run):
    rng = np.random.default_rng(1)
    colour, var, f = denoise_ref.random_inputs(rng, 37, 29)
    out, rgba, out_var = run(colour, var, f, 0)
    assert same_bits(out, colour) and same_bits(out_var, var)
    assert np.array_equal(rgba, denoise_ref.quantise(colour))


def check_a_constant_image_stays_constant(run):
    h, w = 48, 40
    f = {"albedo": np.full((h, w, 3), 0.73), "normal": np.tile([0.0, 0.6, 0.8], (h, w, 1)), "depth": np.full((h, w), 12.5),
         "alpha": np.ones((h, w))}
    colour = np.tile([0.31, 1.7, 0.052], (h, w, 1))
    var = np.full((h, w, 3), 1e-3)
    for v in (None, var):
        out, _, _ = run(colour, v, f, 5)
        # 25 taps of normalised weights: the sum of w c over the sum of w, each within a few ulp of c
        assert np.all(np.abs(out - colour) <= 32 * np.spacing(colour)), np.abs(out - colour).max()


def check_alpha_zero_pixels_pass_through_and_reach_no_neighbour(run):
    rng = np.random.default_rng(2)
    colour, var, f = denoise_ref.random_inputs(rng, 37, 29)
    sky = f["alpha"] == 0.0
    assert sky.sum() > 50
    out, _, out_var = run(colour, var, f, 4)
    assert same_bits(out[sky], colour[sky]) and same_bits(out_var[sky], var[sky])
    other = colour.copy()
    other[sky] = rng.exponential(50.0, size=(int(sky.sum()), 3))
    f2 = dict(f, albedo=f["albedo"].copy(), normal=f["normal"].copy(), depth=f["depth"].copy())
    f2["albedo"][sky], f2["normal"][sky], f2["depth"][sky] = 0.9, [0.0, 0.0, 1.0], 5.0
    out2, _, _ = run(other, var, f2, 4)
    assert same_bits(out2[~sky], out[~sky])
    assert same_bits(out2[sky], other[sky])


def check_no_colour_crosses_an_edge_between_orthogonal_normals(run):
    rng = np.random.default_rng(3)
    h, w = 40, 48
    left = np.zeros((h, w), dtype=bool)
    left[:, : w // 2] = True
    normal = np.where(left[..., None], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]) * np.ones((h, w, 1))
    f = {"albedo": np.full((h, w, 3), 0.5), "normal": normal, "depth": np.full((h, w), 10.0), "alpha": np.ones((h, w))}
    colour = rng.exponential(1.0, size=(h, w, 3))
    out, _, _ = run(colour, None, f, 5)
    other = colour.copy()
    other[~left] += 100.0
    out2, _, _ = run(other, None, f, 5)
    assert same_bits(out2[left], out[left])                             # w_n = 0 exactly across the edge
    assert np.all(out2[~left] > 90.0) and np.all(out[left] < 20.0)
    assert out[left].std() < 0.5 * colour[left].std()              # ... while each side was smoothed


def check_a_variance_that_is_not_finite_is_treated_as_absent(run):
    rng = np.random.default_rng(4)
    colour, _, f = denoise_ref.random_inputs(rng, 37, 29, with_variance=False)
    plain, _, _ = run(colour, None, f, 3)
    for bad in (np.inf, np.nan):
        out, _, out_var = run(colour, np.full(colour.shape, bad), f, 3)
        assert same_bits(out, plain)
        assert not np.isfinite(out_var).any()
    # one pixel without a variance among pixels that have one: it is filtered with w_l = 1, and keeps its own variance
    var = np.full(colour.shape, 0.04)
    var[10, 10] = np.inf
    f1 = dict(f, alpha=np.ones_like(f["alpha"]))
    out, _, out_var = run(colour, var, f1, 1)
    want, _, want_var = denoise_ref.denoise(colour, var, f1, 1)
    assert same_bits(out, want) and same_bits(out_var, want_var)
    assert np.isinf(out_var[10, 10]).all() and np.isfinite(out_var[10, 11]).all()


PROPERTIES = [check_zero_iterations_is_the_identity, check_a_constant_image_stays_constant, check_alpha_zero_pixels_pass_through_and_reach_no_neighbour,
              check_no_colour_crosses_an_edge_between_orthogonal_normals, check_a_variance_that_is_not_finite_is_treated_as_absent]


# ---- locality

LOCALITY_ITERATIONS = 2
LOCALITY_SIZE = (70, 41)
LOCALITY_CROP = (slice(3, 36), slice(5, 58))     # rows, columns of the 70x41 frame: an origin off the device's 32x8 blocks, 53x33 pixels
# Pass i's taps reach 2 * 2^i pixels, k passes 2 * (2^k - 1).  The 3x3 window of the centre's variance adds nothing to that: it reads the previous
# pass's variances one pixel around the CENTRE (a tap's weight uses the centre's scale, not the tap's own), well inside the taps' reach.  So a
# pixel with that many pixels between it and the crop's edge is the whole frame's, bit for bit, and one with a pixel fewer is not.
LOCALITY_MARGIN = 2 * (2 ** LOCALITY_ITERATIONS - 1)


def interior(a, margin):
    return a[margin:a.shape[0] - margin, margin:a.shape[1] - margin]


def locality_results(run, with_variance=True):
    """(the whole frame's result cut to the crop, the crop's own result), each (linear, rgba8, variance)."""
    colour, var, f = frame(LOCALITY_SIZE, with_variance)
    cut = lambda a: None if a is None else a[LOCALITY_CROP]
    whole = run(colour, var, f, LOCALITY_ITERATIONS)
    part = run(cut(colour), cut(var), {k: cut(v) for k, v in f.items()}, LOCALITY_ITERATIONS)
    return tuple(cut(a) for a in whole), part


def check_locality(run, with_variance):
    whole, part = locality_results(run, with_variance)
    assert min(interior(part[0], LOCALITY_MARGIN).shape[:2]) >= 5
    for k, (a, b) in enumerate(zip(part, whole)):
        assert same(None if a is None else interior(a, LOCALITY_MARGIN), None if b is None else interior(b, LOCALITY_MARGIN)), k
    # ... and the margin is not generous: one pixel further out the crop's edge is felt
    assert not same(interior(part[0], LOCALITY_MARGIN - 1), interior(whole[0], LOCALITY_MARGIN - 1))
    if with_variance:
        assert not same(interior(part[2], LOCALITY_MARGIN - 1), interior(whole[2], LOCALITY_MARGIN - 1))


# ---- the farthest tap

def far_tap_frame(transposed=False):
    """129x7 (or 7x129) of one wall — one normal, one depth, one albedo, no sky — and random colours: the only tap of pass 8 (stride 128) that lies
    inside the image joins column 0 and column 128, and here it weighs as much as the bell allows.  (colour, variance, features), read-only."""
    rng = np.random.default_rng(129)
    h, w = (129, 7) if transposed else (7, 129)
    f = {"albedo": np.full((h, w, 3), 0.6), "normal": np.tile([0.0, 0.6, 0.8], (h, w, 1)), "depth": np.full((h, w), 9.0), "alpha": np.ones((h, w))}
    colour = rng.exponential(1.0, size=(h, w, 3))
    return _freeze(colour, colour * colour * 0.09, f)


def check_far_tap(run, transposed=False):
    """Eight passes over far_tap_frame equal the numpy restatement; and, in the restatement itself, the eighth pass over the seventh's result gives
    pixel 0 of the long axis another value than it does in the frame cut to 128: the stride-128 tap weighs there."""
    colour, var, f = far_tap_frame(transposed)
    cut = (slice(0, 128), slice(None)) if transposed else (slice(None), slice(0, 128))
    first = (0, slice(None)) if transposed else (slice(None), 0)
    middle = (slice(1, 128), slice(None)) if transposed else (slice(None), slice(1, 128))
    for v in (var, None):
        assert_same_results(run(colour, v, f, 8), denoise_ref.denoise(colour, v, f, 8))
        c7, _, v7 = denoise_ref.denoise(colour, v, f, 7)
        # the pass alone, at the defaults (sigma_normal 64 is 6 squarings); the one albedo of the wall scales both sides alike
        eighth = lambda c, v, f: denoise_ref._pass(c, v, f["normal"], f["depth"], f["alpha"], 128, denoise_ref.DEFAULTS["sigma_luminance"], 6,
                                                   denoise_ref.DEFAULTS["sigma_depth"])[0]
        whole, part = eighth(c7, v7, f), eighth(c7[cut], None if v7 is None else v7[cut], {k: a[cut] for k, a in f.items()})
        assert not np.array_equal(whole[first], part[first])
        assert same(whole[middle], part[middle])                   # ... and no other pixel of the cut frame has a tap beyond it
