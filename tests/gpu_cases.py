"""What the GPU tests of the adaptive entry points share (tests/test_gpu_adaptive*.py, tests/test_gpu_preview.py, tests/test_gpu_region.py): the
kernel-form switch, the scenes, the two frames every bit-for-bit comparison runs on, the cache of uninterrupted renders and the comparison itself.
The `scenes` and `fresh` fixtures stay in each test module, at module scope: a module builds its own scenes and renders its own references."""
import os

import numpy as np

from rttnw_amd import library
from rttnw_amd import scene as S

# case 1: the parameters of test_gpu_adaptive.py::test_stopping_rule_prefix_and_launch_split, on a 40x24 frame: 15 tiles, so 2 ranks have
# unequal shares and 8 ranks have pad tiles
CASE1 = dict(name="simple_light", w=40, h=24, B=16, cap=128, rel=0.1, ab=0.005, spp_chunk=2)
# case 2: a frame that is no multiple of 8 (45x37: 30 tiles, 8 per rank of 4), test_pixels_compose_from_plain_passes' parameters
CASE2 = dict(name="cornell_box", w=45, h=37, B=16, cap=64, rel=0.15, ab=0.01, spp_chunk=4)
# a tolerance under which case 1 stops most pixels after their first pass and leaves the others spread over the 2nd .. 7th
LOOSE_REL, LOOSE_ABS = 0.5, 0.02


def use_kernel(monkeypatch, kernel):
    """RTTNW_KERNEL for this test: a kernel form's name, or None for the one the scene takes by itself."""
    if kernel:
        monkeypatch.setenv("RTTNW_KERNEL", kernel)
    else:
        monkeypatch.delenv("RTTNW_KERNEL", raising=False)


def build_scenes(gpu, names):
    lib = library.scenes()
    return {name: S.build(gpu, lib, name, S.load_earth() if name == "final_scene" else None) for name in names}


def setup_case(scenes, c, precision):
    sc, setup = scenes[c["name"]]
    cam, p = S.params_for(setup, c["w"], c["h"], c["cap"], precision=precision, spp_chunk=c["spp_chunk"])
    return sc, cam, p


def fresh_cache(render_one):
    """get(case, precision, kernel=None, **over): `render_one(case with over laid over it, precision)`, computed once per (case, precision, kernel
    form) under the default launch split, shared by the tests and never written to."""
    cache = {}

    def get(case, precision, kernel=None, **over):
        c = dict(case, **over)
        key = (tuple(sorted(c.items())), precision, kernel)
        if key not in cache:
            assert os.environ.get("RTTNW_KERNEL") == kernel and "RTTNW_CHUNK_SUM_BUDGET" not in os.environ
            out = render_one(c, precision)
            for a in out:
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            cache[key] = out
        return cache[key]
    return get


def same_outputs(got, ref, where=None, what="", state=True):
    """(linear, rgba8, spp, stderr[, stats, state]) bit for bit (+inf equal to +inf, NaN to NaN): at the pixels `where`, or, by default, everywhere —
    and then the state too, when both carry one and `state` is not turned off."""
    at = (lambda a: a) if where is None else (lambda a: a[where])
    assert np.array_equal(at(got[0]), at(ref[0])), (what, "linear", np.abs(at(got[0]) - at(ref[0])).max())
    assert np.array_equal(at(got[1]), at(ref[1])), (what, "rgba8")
    assert np.array_equal(at(got[2]), at(ref[2])), (what, "samples", int((at(got[2]) != at(ref[2])).sum()))
    assert np.array_equal(at(got[3]), at(ref[3]), equal_nan=True), (what, "stderr")
    if state and where is None and len(got) > 5 and len(ref) > 5:
        assert np.array_equal(got[5], ref[5], equal_nan=True), (what, "state", int((got[5] != ref[5]).sum()))


def samples(stats):
    return sum(x.samples for x in stats) if isinstance(stats, list) else stats.samples


def hist(spp):
    return {int(k): int(v) for k, v in zip(*np.unique(spp, return_counts=True))}
