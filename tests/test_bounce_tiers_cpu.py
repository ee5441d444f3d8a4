"""The re-anchored per-bounce checker (tests/util.py compare_paths_reanchored) checked on the host build of the tracing core
(tests/hostsim): it passes the f32 and f64 cores, finds nothing at all where the core performs the oracle's operations, and fails on
records corrupted in one place.  The device kernels are held to it in tests/test_gpu_bounce_tiers.py."""
import ctypes as C

import numpy as np
import pytest

import util
from rttnw_amd import abi

SCENES = ["cornell_box", "smoke_cornell_box", "final_scene", "random_scene"]


def _probe_fn(hostsim):
    fn = hostsim.lib.hostsim_probe_path
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(abi.CameraDesc), C.POINTER(abi.Params), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                   C.c_uint32]
    return fn


def _setup(hostsim, oracle, scenes_lib, earth, name, precision, n_pairs=120):
    sh, setup = util.build(hostsim, scenes_lib, name, earth)
    so, _ = util.build(oracle, scenes_lib, name, earth)
    cam, p = util.params_for(setup, 96, 96, 8, seed=21, precision=precision)
    rng = np.random.default_rng(17)
    pairs = [(int(rng.integers(96)), int(rng.integers(96)), int(rng.integers(8))) for _ in range(n_pairs)]
    fn = _probe_fn(hostsim)
    return (lambda x, y, s: util.product_probe_tail(fn, hostsim, sh, cam, p, x, y, s)), so, cam, p, pairs


@pytest.mark.parametrize("precision", [abi.F32, abi.F64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", SCENES)
def test_hostsim_bounces_equal_oracle_reanchored(hostsim, oracle, scenes_lib, earth, name, precision):
    """Every bounce of 120 paths of the host core at the tier's own bounds (K = 8, w = 32; util.compare_paths_reanchored) — the f32
    core with f32 eps, the f64 core with f64 eps, at every depth.  (The host core divides and takes square roots in IEEE arithmetic,
    so it sits well inside what the device kernels are allowed.)  Measured: f32 <= 3.9 eps x scale beyond the hull (final_scene t), f64
    <= 0.47 (final_scene normal), no flip."""
    probe, so, cam, p, pairs = _setup(hostsim, oracle, scenes_lib, earth, name, precision)
    res = util.compare_paths_reanchored(probe, so, cam, p, pairs, util.EPS_F32 if precision == abi.F32 else util.EPS_F64)
    assert res.paths == 120 and res.bounces >= 200 and len(res.mat_map) >= 3


@pytest.mark.parametrize("name", ["cornell_box", "smoke_cornell_box", "random_scene"])
def test_hostsim_f64_is_exact_under_the_strict_checker(hostsim, oracle, scenes_lib, earth, name):
    """Where the host f64 core performs the oracle's operations in its order (no contraction on the host; no transformed group of
    spheres, whose world-space copies only the device's strict build tests in the reference's frame) the checker's strict form —
    no perturbation, no flip — finds nothing beyond 1e-12: if it did, the checker would be wrong, not the core."""
    probe, so, cam, p, pairs = _setup(hostsim, oracle, scenes_lib, earth, name, abi.F64)
    res = util.compare_paths_reanchored(probe, so, cam, p, pairs, util.EPS_F64, strict_tol=1e-12, max_flip_share=0.0)
    assert not res.flips and max(res.excess.values()) <= 1e-12 and res.bounces >= 250


def _mutate(kind, recs, tail):
    """Corrupt the probe's output of one path in one place; None when this path has nothing to corrupt that way."""
    recs, tail = recs.copy(), tail.copy()
    n = len(recs)
    if kind == "t" and n >= 2:
        recs[1, 0] *= 1.0 + 8.0 * 2.0 ** -24
    elif kind == "normal" and n >= 1:
        i = 4 + int(np.argmax(np.abs(recs[0, 4:7])))
        recs[0, i] = -recs[0, i]
    elif kind == "material" and n >= 2 and recs[0, 7] != recs[1, 7]:
        recs[0, 7], recs[1, 7] = recs[1, 7], recs[0, 7]
    elif kind == "attenuation" and n >= 2 and recs[0, 19] > 0.0:
        recs[0, 19] *= 1.0 + 2.0 ** -20
    elif kind == "drop" and n >= 3:
        recs = np.delete(recs, 1, axis=0)
    elif kind == "tail_green" and n >= 1 and tail[1] > 0.0:
        tail[1] *= 1.0 + 2.0 ** -20
    elif kind == "truncate" and n >= 3 and recs[1, 19] >= 0.0:
        recs = recs[:2]                      # ... as if the second bounce's scattered ray had missed: the tail made consistent with that
        tail[0:3], tail[3] = 0.0, 2.0
    else:
        return None
    return recs, tail


@pytest.mark.parametrize("kind", ["t", "normal", "material", "attenuation", "drop", "tail_green", "truncate"])
def test_checker_fails_on_a_record_corrupted_in_one_place(hostsim, oracle, scenes_lib, earth, kind):
    """The checker is sharp: the host f64 core's records pass it (test above), and the same records with ONE value changed do not —
    t scaled by (1 + 8 * 2^-24), a normal component's sign flipped, two bounces' materials swapped, attenuation.r scaled by (1 + 2^-20),
    a middle bounce dropped, the tail's green channel scaled by (1 + 2^-20), a path cut short where the oracle's continues.  Each
    is checked with the contracted tier's settings (f64 eps, perturbations and allowed flips on), the weaker of the two."""
    probe, so, cam, p, pairs = _setup(hostsim, oracle, scenes_lib, earth, "cornell_box", abi.F64, n_pairs=60)
    done = []

    def corrupted(x, y, s):
        recs, tail = probe(x, y, s)
        if not done:
            m = _mutate(kind, recs, tail)
            if m is not None:
                done.append((x, y, s))
                return m
        return recs, tail
    util.compare_paths_reanchored(probe, so, cam, p, pairs, util.EPS_F64)   # (the same pairs, untouched, pass)
    with pytest.raises(AssertionError):
        util.compare_paths_reanchored(corrupted, so, cam, p, pairs, util.EPS_F64)
    assert done, kind
