"""The optional outputs of the blocking image-filter calls on the MI355X: rttnw_denoise, rttnw_reconstruct, rttnw_denoise_nlm, rttnw_denoise_select,
rttnw_denoise_regress, rttnw_temporal_accumulate, rttnw_temporal_variance, rttnw_temporal_clamp and rttnw_temporal_probe, straight through the C ABI
(rttnw_amd/render.py always asks for every output).  Each call is made once with every output and kernel_ms, then once per output with only that
output non-NULL and kernel_ms NULL: the single output equals the full call's bit for bit — an output's copy depends on no other output having been
asked for — and behind every caller array stands a guard band of a sentinel that no copy may touch — each copy has the length of its array.
24x20: no multiple of the 64x4 and 32x8 blocks or of the NLM / select tiles, and narrower than one block.  With a history where the call takes
one, with and without variances where it has that choice.  What the kernels compute is held by the tests/test_gpu_<filter>.py files."""
import ctypes as C
import re

import numpy as np
import pytest

from abi_cases import HEADER
from rttnw_amd import abi
from rttnw_amd import scene as S

pytestmark = pytest.mark.gpu
W, H = 24, 20
GUARD = 64                                    # elements behind every output array
SENTINEL = {np.float64: -12345.678, np.uint8: 0xA5}
PER_PIXEL = {"depth": 1, "alpha": 1, "valid": 1, "prev_length": 1, "prev_depth": 1, "prev_alpha": 1, "out_valid": 1, "out_blend": 1, "out_fit": 1,
             "out_length": 1, "out_clipped": 1, "out_multiplier": 1, "out_prev_xy": 2, "out_rgba8": 4}   # every other array: 3
BLOCKS = {"rttnw_denoise_params": abi.Denoise, "rttnw_nlm_params": abi.Nlm, "rttnw_select_params": abi.Select, "rttnw_regress_params": abi.Regress,
          "rttnw_temporal_params": abi.Temporal, "rttnw_variance_params": abi.Variance, "rttnw_clamp_params": abi.Clamp,
          "rttnw_sampling_params": abi.Sampling}
VARIANCES = ("variance_rgb", "var_a", "var_b", "prev_variance_rgb")


def _prototype(name):
    proto = re.search(r"\bint rttnw_%s\((.*?)\);" % name, HEADER, flags=re.S).group(1)
    return [re.match(r"(.+?)\s*(\w+)$", a.strip()).groups() for a in " ".join(proto.split()).split(",")]


@pytest.fixture(scope="module")
def frame():
    """Seeded inputs by argument name: colours in [0, 1), small positive variances, unit normals, positive depth, alpha 0 / 1; the history is seen
    through the same camera and has the frame's own features, so its taps are accepted, and lengths 1 .. 5."""
    rng = np.random.default_rng(20)
    n = W * H
    normal = rng.normal(size=(n, 3))
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    f = {"albedo": rng.uniform(0.1, 1.0, n * 3), "normal": normal.ravel(), "depth": rng.uniform(1.0, 5.0, n),
         "alpha": (rng.uniform(size=n) < 0.8).astype(np.float64), "valid": (rng.uniform(size=n) < 0.5).astype(np.uint8),
         "prev_length": rng.integers(1, 6, n).astype(np.float64)}
    for name in ("linear_rgb", "half_a", "half_b", "prev_linear_rgb"):
        f[name] = rng.uniform(0.0, 1.0, n * 3)
    for name in VARIANCES:
        f[name] = rng.uniform(0.001, 0.05, n * 3)
    f["prev_moment2_rgb"] = f["prev_linear_rgb"] ** 2 + rng.uniform(0.0, 0.02, n * 3)
    f.update(prev_normal=f["normal"], prev_depth=f["depth"], prev_alpha=f["alpha"])
    return {k: np.ascontiguousarray(v) for k, v in f.items()}


def _outputs(name):
    return [arg for _, arg in _prototype(name) if arg.startswith("out_")]


def _run(gpu, name, frame, with_variance, blocks, wanted, want_ms):
    """One call of rttnw_<name>: the outputs in `wanted` get guarded arrays, the others NULL.  Returns {output: (array, its length)} and kernel_ms."""
    cam = S.camera_desc(lookfrom=(0, 0, 5), lookat=(0, 0, 0), vfov=40.0, aspect=W / H)
    ms = C.c_double(-1.0)
    keep, out, args = [cam], {}, []
    for ctype, arg in _prototype(name):
        base = ctype.replace("const ", "").replace("*", "").strip()
        if arg in ("width", "height"):
            args.append(W if arg == "width" else H)
        elif base == "rttnw_camera_desc":
            args.append(C.byref(cam))
        elif base in BLOCKS:
            keep.append(BLOCKS[base](**blocks.get(arg, {})))
            args.append(C.byref(keep[-1]))
        elif arg == "kernel_ms":
            args.append(C.byref(ms) if want_ms else None)
        elif arg.startswith("out_"):
            if arg in wanted:
                dtype = np.uint8 if "uint8_t" in ctype else np.float64
                n = W * H * PER_PIXEL.get(arg, 3)
                out[arg] = (np.full(n + GUARD, SENTINEL[dtype], dtype=dtype), n)
                args.append(out[arg][0].ctypes.data)
            else:
                args.append(None)
        else:
            args.append(None if arg in VARIANCES and not with_variance else frame[arg].ctypes.data)
    assert getattr(gpu, name)(*args) == 0, gpu.last_error().decode()
    return out, ms.value


CALLS = [  # (entry point, has the with / without variance choice, parameter blocks that switch every stage on): the eight wrappers, denoise.hip's twice
    ("denoise", True, {"d": {"iterations": 3}}),
    ("reconstruct", True, {"d": {"iterations": 3}}),
    ("denoise_nlm", True, {"d": {"search_radius": 3, "patch_radius": 1}}),
    ("denoise_select", True, {"dn": {"iterations": 2}, "nl": {"search_radius": 3, "patch_radius": 1}, "sel": {"use_default_margin": 1}}),
    ("denoise_regress", True, {"g": {"search_radius": 3, "patch_radius": 1, "features": 7, "demodulate": 1}}),
    ("temporal_accumulate", True, {}),
    ("temporal_variance", False, {}),
    ("temporal_clamp", False, {"k": {"gamma": 0.5}}),
    ("temporal_probe", False, {}),
]
CASES = [(name, v, blocks) for name, choice, blocks in CALLS for v in ((True, False) if choice else (False,))]


@pytest.mark.parametrize("name,with_variance,blocks", CASES, ids=["%s-%s" % (c[0], "var" if c[1] else "novar") for c in CASES])
def test_each_output_alone_equals_the_full_call_and_no_copy_leaves_its_array(gpu, frame, name, with_variance, blocks):
    names = _outputs(name)
    full, ms = _run(gpu, name, frame, with_variance, blocks, names, True)
    assert ms > 0.0, "kernel_ms is reported"
    for arg in names:
        alone, no_ms = _run(gpu, name, frame, with_variance, blocks, [arg], False)
        assert no_ms == -1.0 and list(alone) == [arg]
        for (a, n), what in ((full[arg], "the full call"), (alone[arg], "alone")):
            assert (a[n:] == SENTINEL[a.dtype.type]).all(), (arg, what, "wrote behind the array")
        assert full[arg][0].tobytes() == alone[arg][0].tobytes(), (arg, "differs from the full call's")
        untouched = bool((full[arg][0] == SENTINEL[full[arg][0].dtype.type]).all())
        # an output that the call does not have in this form stays as the caller left it: the filtered variance without a variance to filter
        assert untouched == (arg == "out_variance_rgb" and not with_variance and name != "temporal_variance" and name != "temporal_clamp"), arg

