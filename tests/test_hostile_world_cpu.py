"""The hostile world (tests/hostile_world.py) on the reference side, without a GPU: the host build of the product's core and lowering
(tests/hostsim) against the oracle rendering the same items as a FLAT LIST — no box anywhere, the exact f64 closest hit of every ray.
The render RNG does not depend on how a world is grouped, so tree and list make the same rays.  tests/test_gpu_hostile_geometry.py holds
the device to the same reference."""
import ctypes as C

import numpy as np
import pytest

import hostile_world as hw
import util
from oracle import rto
from rttnw_amd import abi

WORLD = pytest.mark.parametrize("world", range(len(hw.WORLDS)), ids=hw.WORLD_IDS)


@pytest.fixture(scope="module")
def oracle_lists(oracle):
    """Per world: the oracle's flat-list renders of both cameras in f64 as [(linear, rays)].  Made once, never written to."""
    out = []
    for scale, shift in hw.WORLDS:
        so, _ = hw.scene(oracle, scale, shift, tree=False)
        p = hw.params(abi.F64, scale, collect_counters=1)
        per_cam = []
        for cam in hw.cameras(scale, shift):
            lin, _, st = rto.render(so, cam, p)
            lin.setflags(write=False)
            per_cam.append((lin, st.rays))
        out.append(per_cam)
    return out


@WORLD
@pytest.mark.parametrize("quant", [None, "1"], ids=["f32_records", "quantised_records"])
def test_core_on_a_tree_equals_the_oracle_on_a_list(hostsim, oracle_lists, world, quant, monkeypatch):
    """F64, the items inside a bvh_tree, walked through the f32 node records and through the 8-bit quantised ones (HOSTSIM_QUANT=1: what
    the decoupled kernel walks): every pixel within 1e-12 of the flat-list oracle and the same number of rays, for both cameras — boxes
    that are flat, inverted, 1e6 away or 1e-3 small cull nothing they should not."""
    scale, shift = hw.WORLDS[world]
    if quant is None:
        monkeypatch.delenv("HOSTSIM_QUANT", raising=False)
    else:
        monkeypatch.setenv("HOSTSIM_QUANT", quant)
    sh, _ = hw.scene(hostsim, scale, shift)
    p = hw.params(abi.F64, scale, collect_counters=1)
    for cam, (lo, rays) in zip(hw.cameras(scale, shift), oracle_lists[world]):
        lin, st = util.hostsim_render(hostsim, sh, cam, p)
        assert np.abs(lin - lo).max() <= 1e-12, np.abs(lin - lo).max()
        assert st.rays == rays
        assert lo.max() > 1.0 and lo.std() > 0.05   # the world is lit and in view


@WORLD
def test_inverted_bounds_are_invisible_in_a_reference_tree_and_visible_in_the_product(hostsim, oracle, world, monkeypatch):
    """A sphere of negative radius and a cube from swapped corners have bounds with min > max, which the reference stores literally
    (hittable.rs:125-130); Bound::hit (bound.rs:13-32) then never passes them, so inside a BvhTree such an object cannot be hit, while in
    a List it can.  The product normalises its tree boxes (SURVEY's rule for quirk Q2: its own correct, conservative boxes): tree or
    list, it shows what the reference's LIST shows.  Both are on record here, on a world of such objects alone (plus ground and light):
    the oracle's tree render differs from its list render and makes fewer rays; the host build of the product on the tree equals the
    oracle on the list."""
    monkeypatch.delenv("HOSTSIM_QUANT", raising=False)
    scale, shift = hw.WORLDS[world]
    s_list, _ = hw.scene(oracle, scale, shift, tree=False, kinds=hw.INVERTED)
    s_tree, _ = hw.scene(oracle, scale, shift, tree=True, kinds=hw.INVERTED)
    s_host, its = hw.scene(hostsim, scale, shift, tree=True, kinds=hw.INVERTED)
    assert len(its) == 42
    p = hw.params(abi.F64, scale, collect_counters=1)
    for cam in hw.cameras(scale, shift):
        lo, _, st_l = rto.render(s_list, cam, p)
        lt, _, st_t = rto.render(s_tree, cam, p)
        differ = (np.abs(lt - lo).max(axis=2) > 1e-12).mean()
        assert differ > 0.01 and st_t.rays < st_l.rays, (differ, st_t.rays, st_l.rays)
        lin, st = util.hostsim_render(hostsim, s_host, cam, p)
        assert np.abs(lin - lo).max() <= 1e-12 and st.rays == st_l.rays


@WORLD
def test_host_lowering_gives_every_item_a_tight_leaf_box(hostsim, world):
    """Every hittable pushed into the tree: its bounds over times 0 .. 1 (rttnw_hittable_bounds, normalised per axis to (min, max) — the
    inverted ones too) lie inside some leaf slot box of the lowered tree, each face of which is at most 4 f32 steps outside them
    (scene_lower.cpp set_box rounds outward and pads two ulps: 3 steps at most; a wrapped cube's box carries a guard of 1e-9 of the
    coordinates its transform handled, far below a step).  A constant_medium is no leaf: its boundary is tested after the walk, for every
    ray, so no box can cull it — the three media are the only items without a leaf box."""
    scale, shift = hw.WORLDS[world]
    sh, its = hw.scene(hostsim, scale, shift)
    n4, root = util.nodes_of(hostsim, sh, wide=True)
    leaves, need, inst_need = hw.check_trees(n4, root)
    dims = (C.c_uint32 * 8)()
    hostsim.lib.hostsim_scene_dims(sh.handle, dims)
    assert dims[7] == need + 1 + inst_need + 1   # the stack bound: the top tree's pending children, a sentinel + a wrapped cube's tree's, one spare
    solid = [(k, i) for k, i in its if k != "medium"]
    assert len(its) == 511 and len(solid) == 508 and len(leaves) == len(solid)   # one record per leaf
    assert hw.items_without_a_tight_leaf_box(sh, solid, n4) == []
    assert [k for k, _, _, _ in hw.items_without_a_tight_leaf_box(sh, its, n4)] == ["medium"] * 3
