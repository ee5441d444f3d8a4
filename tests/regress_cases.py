"""What the tests of rttnw_denoise_regress share (tests/test_regress_cpu.py on the host harness, tests/test_gpu_regress.py on the device): the
frames and parameter sets both are held to, the inputs, and the checks of the properties both must have."""
import numpy as np

import nlm_ref
import regress_ref
from nlm_cases import crop_interior, same_bits

# 1x1 and 3x5 are smaller than every window (all halo); 17x16, 33x18 and 37x29 cross the device's 16-pixel tiles, 35x33 its 32-pixel tile in both axes
CPU_FRAMES = [(1, 1), (3, 5), (17, 16), (37, 29)]
GPU_FRAMES = [(1, 1), (3, 5), (33, 18), (37, 29), (35, 33)]
CPU_RADII = [(1, 1), (7, 3), (2, 4)]
GPU_RADII = [(1, 1), (7, 3), (16, 4)]            # the last takes the device's 16-pixel tile under every mask
CPU_MASKS = [0, 1, 2, 4, 7]
GPU_MASKS = [0, 1, 4, 7]                         # the 32-pixel tile (0, 1, 4: d <= 4) and the 16-pixel tile (7) at the default radii
RIDGES = [0.0, 1e-12, 1e-1]                      # 0: the library default


def inputs(seed, w, h, with_variance):
    """(half_a, half_b, var_a, var_b, features) of a w x h frame: tests/nlm_ref.py's noisy halves beside feature maps with a texture, a depth step, sky
    and fractional alphas."""
    rng = np.random.default_rng(seed)
    a, b, va, vb = nlm_ref.random_inputs(rng, w, h, with_variance)
    return a, b, va, vb, regress_ref.random_features(rng, w, h)


def assert_same_outputs(got, want, what):
    for name in regress_ref.OUTPUTS:
        assert same_bits(got[name], want[name]), (name,) + tuple(what) + (float(np.nanmax(np.abs(got[name].astype(np.float64) - want[name]))),)


def swapped_equal(one, other):
    """`other` is the call with (half_a, var_a) and (half_b, var_b) exchanged: the image, its RGBA8, the error and the fit count are the same bits,
    the two fitted halves change places."""
    for name in ("linear", "rgba8", "error", "fit"):
        assert same_bits(one[name], other[name]), name
    assert same_bits(one["half_a"], other["half_b"]) and same_bits(one["half_b"], other["half_a"])
    assert not same_bits(one["half_a"], one["half_b"])


def crop_features(features, crop):
    return {name: features[name][crop] for name in regress_ref.FEATURES}


def locality(run, a, b, va, vb, features, crop, r, f, short, **kw):
    """Property 3 under `run` (the host harness or the device): the interior of a crop taken with a margin of r + f + 1 equals the same pixels of the
    whole frame's result in every output; with the margin `short` the crop's edge is felt."""
    m = r + f + 1
    whole = run(a, b, va, vb, features, search_radius=r, patch_radius=f, **kw)
    part = run(a[crop], b[crop], None if va is None else va[crop], None if vb is None else vb[crop], crop_features(features, crop),
               search_radius=r, patch_radius=f, **kw)
    assert min(crop_interior(part["linear"], m).shape[:2]) >= 5
    for name in regress_ref.OUTPUTS:
        assert same_bits(crop_interior(part[name], m), crop_interior(whole[name][crop], m)), name
    assert not same_bits(crop_interior(part["linear"], short), crop_interior(whole["linear"][crop], short))
