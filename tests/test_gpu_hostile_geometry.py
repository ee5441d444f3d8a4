"""Every kernel form and every builder on hostile geometry (tests/hostile_world.py), against the oracle rendering the same items as a
flat list: no box anywhere, the exact f64 closest hit of every ray (tests/test_hostile_world_cpu.py holds the host build of the
same core to it: <= 4.5e-16 on every pixel).  The device compiles that core with -ffp-contract=fast in two of its three builds, OCML
quotients and v_min / v_max, and only the device has the LDS-resident node path, the decoupled kernel's ray arena and quantised
64-byte records, morton_kernel, the device SAH bins and the collapse kernels: flat boxes, boxes of min > max, a child that spans its
node, coordinates of 1e6 and 1e-3 and rays with a zero direction component meet them here.

Per (world, precision): the scene once per builder, both cameras under each forced form (RTTNW_KERNEL): 18 renders of 33 x 33 x 3."""
import numpy as np
import pytest

import hostile_world as hw
import util
from oracle import rto
from rttnw_amd import abi, render

pytestmark = pytest.mark.gpu

BUILDERS = [("sah", abi.BVH_HOST_SAH), ("lbvh", abi.BVH_DEVICE_LBVH), ("dsah", abi.BVH_DEVICE_SAH)]
FORMS = ("plain", "plainglobal", "wave")
N_PIXELS = hw.WIDTH * hw.HEIGHT
WORLD = pytest.mark.parametrize("world", range(len(hw.WORLDS)), ids=hw.WORLD_IDS)

# Measured on an MI355X (profiles/LEDGER.md, "hostile geometry"): the largest share of the 1089 pixels, over the forms, builders and
# cameras of a world.  F64: (beyond 1e-9 from the oracle's list render, differing at all between two forms).
F64_MEASURED = {"origin": (0.0, 0.0), "milli": (0.0, 0.0), "1e6": (0.0, 0.0)}
# F32: (beyond 1e-3 from the oracle's list render — None in the 1e6 world, differing at all between two forms)
F32_MEASURED = {"origin": (3 / 1089, 0.0), "milli": (3 / 1089, 0.0), "1e6": (None, 0.0)}


@pytest.fixture(scope="module")
def scenes(gpu):
    """get(world, builder) -> (Scene, items): each world built once per builder for the whole module."""
    made = {}

    def get(world, builder):
        if (world, builder) not in made:
            scale, shift = hw.WORLDS[world]
            made[(world, builder)] = hw.scene(gpu, scale, shift, bvh=builder)
        return made[(world, builder)]
    return get


@pytest.fixture(scope="module")
def oracle_lists(oracle):
    """Per world and camera: the oracle's flat-list render (linear, RGBA8, rays).  Made once, never written to."""
    out = []
    for scale, shift in hw.WORLDS:
        so, _ = hw.scene(oracle, scale, shift, tree=False)
        p = hw.params(abi.F64, scale, collect_counters=1)
        per_cam = []
        for cam in hw.cameras(scale, shift):
            lin, rgba, st = rto.render(so, cam, p)
            lin.setflags(write=False)
            rgba.setflags(write=False)
            per_cam.append((lin, rgba, st.rays))
        out.append(per_cam)
    return out


def render_all(scenes, world, precision, monkeypatch):
    """{(builder name, form, camera index): (linear, rgba8, rays)}; the forced form is the one that ran (rttnw_stats.reserved bit 0: the
    decoupled kernel; bit 1: node records resident in LDS, which this tree's host build fits)."""
    scale, shift = hw.WORLDS[world]
    p = hw.params(precision, scale, collect_counters=1)
    out = {}
    for bname, builder in BUILDERS:
        sc, _ = scenes(world, builder)
        assert sc.build_info().builder == builder
        for form in FORMS:
            monkeypatch.setenv("RTTNW_KERNEL", form)
            for ci, cam in enumerate(hw.cameras(scale, shift)):
                lin, rgba, st = render.render_host(sc, cam, p)
                assert (st.reserved & 1) == (1 if form == "wave" else 0), (bname, form, st.reserved)
                assert (st.reserved & 2) == 0 or form == "plain", (bname, form, st.reserved)
                if builder == abi.BVH_HOST_SAH:
                    assert ((st.reserved & 2) != 0) == (form == "plain"), (form, st.reserved)
                assert st.samples == N_PIXELS * hw.SPP
                out[(bname, form, ci)] = (lin, rgba, st.rays)
    monkeypatch.delenv("RTTNW_KERNEL")
    return out


def builders_agree(out):
    """A tree never changes a result: within one form the three builders' images are bit-identical, with the same world.hit() calls."""
    for form in FORMS:
        for ci in range(2):
            a = out[("sah", form, ci)]
            for bname in ("lbvh", "dsah"):
                b = out[(bname, form, ci)]
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2], (bname, form, ci, np.abs(a[0] - b[0]).max())


def share(mask):
    return float(mask.mean())


def forms_differ(out):
    """The largest share of pixels on which two forms' images (host-built tree) differ at all, over the cameras."""
    return max(share((out[("sah", f, ci)][0] != out[("sah", g, ci)][0]).any(axis=2))
               for ci in range(2) for f, g in (("plain", "plainglobal"), ("plain", "wave"), ("plainglobal", "wave")))


@WORLD
def test_f64_strict_is_the_oracles_list_render(scenes, oracle_lists, world, monkeypatch):
    """RTTNW_F64_STRICT (nothing contracted, IEEE quotients): every form, every builder, both cameras: every pixel within 1e-12 of the
    oracle's flat-list render, RGBA8 identical, the same number of rays, and all nine images of a camera bit-identical."""
    out = render_all(scenes, world, abi.F64_STRICT, monkeypatch)
    for (bname, form, ci), (lin, rgba, rays) in out.items():
        lo, ro, rays_o = oracle_lists[world][ci]
        d = np.abs(lin - lo).max(axis=2)
        where = np.unravel_index(np.argmax(d), d.shape)
        assert d.max() <= 1e-12, (hw.WORLD_IDS[world], ci, form, bname, where, d.max())
        assert np.array_equal(rgba, ro) and rays == rays_o, (ci, form, bname, rays, rays_o)
        assert np.array_equal(lin, out[("sah", "plain", ci)][0]), (ci, form, bname)


@WORLD
def test_f64_builders_agree_and_forms_stay_at_the_oracle(scenes, oracle_lists, world, monkeypatch):
    """RTTNW_F64 (contracted).  Across builders within a form: bit-identical, equal rays.  Across forms: equal rays;
    contraction is the only licence for a remainder: the share of pixels beyond 1e-9 from the oracle's list render and the share that
    differ between two forms are held to twice what an MI355X gave, never more than 1 % (the host build: 0 of 1089 beyond 1e-9).
    Measured (share of 1089 pixels, largest over forms, builders, cameras; beyond 1e-9 / forms differ):
      origin  0 / 0      milli  0 / 0      1e6  0 / 0   (max |delta| 4.4e-16 everywhere, the rays the oracle's)"""
    name = hw.WORLD_IDS[world]
    out = render_all(scenes, world, abi.F64, monkeypatch)
    beyond = max(share(np.abs(lin - oracle_lists[world][ci][0]).max(axis=2) > 1e-9) for (_, _, ci), (lin, _, _) in out.items())
    differ = forms_differ(out)
    worst = max(np.abs(lin - oracle_lists[world][ci][0]).max() for (_, _, ci), (lin, _, _) in out.items())
    print("hostile %s f64: beyond 1e-9 of the oracle %.6f (%d px), forms differ %.6f (%d px), max |delta| %.3g, rays %s (oracle %s)"
          % (name, beyond, round(beyond * N_PIXELS), differ, round(differ * N_PIXELS), worst,
             sorted({r for _, _, r in out.values()}), [o[2] for o in oracle_lists[world]]))
    builders_agree(out)
    for (bname, form, ci), (_, _, rays) in out.items():
        assert rays == out[("sah", "plain", ci)][2], (ci, form, bname, rays)
    m_beyond, m_differ = F64_MEASURED[name]
    assert beyond <= min(2.0 * m_beyond, 0.01), (beyond, m_beyond)
    assert differ <= min(2.0 * m_differ, 0.01), (differ, m_differ)


@WORLD
def test_f32_builders_agree_and_forms_stay_near_the_oracle(scenes, oracle_lists, world, monkeypatch):
    """RTTNW_F32.  Across builders within a form: bit-identical; every pixel finite; the image lit.  At the origin and at scale 1e-3 the
    share of pixels beyond 1e-3 from the oracle's list render is held to four times what an MI355X gave (the margin
    tests/test_gpu_features.py uses for single-sample edge crossings), never more than 2 % (the host build: 0.09 - 0.28 %).
    In the 1e6 world there is no oracle comparison: t_min = 1e-3 is far below an f32 ulp of the coordinates (0.06 - 0.25), a scattered
    ray meets the surface it left again — the host build's f32 is beyond 1e-3 on 53 - 56 % of the pixels (45 % on a first draft of this
    world) with 2.2 times the rays —,
    so f32 there can only be held to itself: the builders agree, the pixels are finite, and the share of pixels on which two forms
    differ stays within four times the measured one — which is none: the three forms render the same bytes there.  At the origin and
    at 1e-3 two forms may differ on 0.2 % of the pixels at most (the bound test_kernel_forms_agree holds f32 to).
    Measured (share of 1089 pixels, largest over forms, builders, cameras; beyond 1e-3 / forms differ):
      origin  3 px = 0.28 % / 0      milli  3 px = 0.28 % / 0      1e6  (608 px = 56 %, 2.2 times the oracle's rays) / 0"""
    name = hw.WORLD_IDS[world]
    out = render_all(scenes, world, abi.F32, monkeypatch)
    differ = forms_differ(out)
    beyond = max(share(np.abs(lin - oracle_lists[world][ci][0]).max(axis=2) > 1e-3) for (_, _, ci), (lin, _, _) in out.items())
    print("hostile %s f32: beyond 1e-3 of the oracle %.6f (%d px), forms differ %.6f (%d px), rays %s (oracle %s)"
          % (name, beyond, round(beyond * N_PIXELS), differ, round(differ * N_PIXELS),
             sorted({r for _, _, r in out.values()}), [o[2] for o in oracle_lists[world]]))
    builders_agree(out)
    for (bname, form, ci), (lin, _, _) in out.items():
        assert np.isfinite(lin).all() and lin.min() >= 0.0 and lin.max() > 1.0, (ci, form, bname)
    m_beyond, m_differ = F32_MEASURED[name]
    if m_beyond is not None:
        assert beyond <= min(4.0 * m_beyond, 0.02), (beyond, m_beyond)
        assert differ <= 2e-3, differ
    else:
        assert differ <= 4.0 * m_differ, (differ, m_differ)


@WORLD
@pytest.mark.parametrize("builder", [abi.BVH_DEVICE_LBVH, abi.BVH_DEVICE_SAH], ids=["lbvh", "dsah"])
def test_device_built_trees_over_hostile_items(gpu, scenes, builder, world):
    """The node records morton_kernel / the device SAH bins and the collapse kernels write over flat and inverted boxes, a leaf as large
    as the root and offsets of 1e6: a well-formed 4-wide tree (util.check_wide_tree) whose deepest walk is what the stack bound says;
    the build repeats byte for byte; its leaf slot boxes are, as a multiset of bytes, the host SAH tree's (both bound a leaf by
    set_box of the same primitive); and every item pushed into the tree has a leaf box at most 4 f32 steps outside its bounds (the
    host lowering: tests/test_hostile_world_cpu.py)."""
    scale, shift = hw.WORLDS[world]
    sc, its = scenes(world, builder)
    bi = sc.build_info()
    assert bi.builder == builder and bi.device_ms > 0
    n4, root = util.nodes_of(gpu, sc, wide=True)
    leaves, need, inst_need = hw.check_trees(n4, root)
    solid = [(k, i) for k, i in its if k != "medium"]   # (a medium is no leaf: its boundary is tested after the walk)
    assert len(leaves) == len(solid) == 508 and len(set(leaves)) == 508
    assert need + 1 + inst_need + 1 == bi.stack_depth   # (inside a wrapped cube's tree: one sentinel and that tree's pending children)
    n2, _ = util.nodes_of(gpu, sc)
    again, _ = hw.scene(gpu, scale, shift, bvh=builder)
    assert util.nodes_of(gpu, again)[0].tobytes() == n2.tobytes() and util.nodes_of(gpu, again, wide=True)[0].tobytes() == n4.tobytes()
    host, _ = scenes(world, abi.BVH_HOST_SAH)
    h4, _ = util.nodes_of(gpu, host, wide=True)
    assert hw.sorted_box_bytes(*hw.leaf_slot_boxes(n4)) == hw.sorted_box_bytes(*hw.leaf_slot_boxes(h4))
    assert hw.items_without_a_tight_leaf_box(sc, solid, n4) == []
