"""What the tests of rttnw_denoise_nlm share (tests/test_nlm_cpu.py on the host harness, tests/test_gpu_nlm.py on the device): the frames and
parameter sets both are held to, and the checks of the two properties both must have."""
import numpy as np

# 1x1 and 3x5 are smaller than every window; 17x16, 33x18 and 37x29 cross the device's 16-pixel tiles in one axis, in both, and twice; they
# cross its 32-pixel tiles in x only, 35x33 in both axes
FRAMES = [(1, 1), (3, 5), (17, 16), (33, 18), (37, 29), (35, 33)]
# the device takes its 32-pixel tile for the first, the second and the last of these, its 16-pixel tile for r 16, f 4
RADII = [(1, 1), (7, 3), (16, 4), (2, 4)]
KS = [0.0, 0.45, 2.0]  # 0: the default


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def crop_interior(a, margin):
    return a[margin:a.shape[0] - margin, margin:a.shape[1] - margin]


def swapped_equal(one, other):
    """`other` is the call with (half_a, var_a) and (half_b, var_b) exchanged: the image, its RGBA8 and the error are the same bits, the two
    filtered halves change places."""
    for name in ("linear", "rgba8", "error"):
        assert same_bits(one[name], other[name]), name
    assert same_bits(one["half_a"], other["half_b"]) and same_bits(one["half_b"], other["half_a"])
    assert not same_bits(one["half_a"], one["half_b"])
