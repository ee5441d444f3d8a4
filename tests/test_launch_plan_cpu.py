"""The launch plan (rttnw_amd/csrc/launch_plan.hpp plan_launch) — which kernel instantiation a scene runs, its block and LDS sizes and bits 0-5 of
rttnw_stats.reserved — is pure host logic over the lowered scene: the facts the GPU suite asserts about those bits, held here on the host build
(tests/hostsim), where no GPU is needed.  The GPU assertions stay where they are (tests/test_gpu_parity.py)."""
import pytest

import util

AUTO, PLAIN, PLAINGLOBAL, WAVE = range(4)                       # launch_plan.hpp KernelForm
SHAPES_FAST, SHAPES_GENERAL, SHAPES_NONE, SHAPES_SINGLE, SHAPES_NONE_NT, SHAPES_SINGLE_NT = range(6)   # rt_core.hpp
LDS_BYTES_PER_CU = 160 * 1024
CATALOGUE = [("cornell_box", 0), ("smoke_cornell_box", 0), ("final_scene", 0), ("spheres_1m", 20000), ("random_scene", 0)]


def plan(hostsim, sc, real_bytes, **kw):
    return util.hostsim_launch_plan(hostsim.lib, sc, real_bytes, **kw)


@pytest.mark.parametrize("real_bytes", [4, 8], ids=["f32", "f64"])
@pytest.mark.parametrize("scene", CATALOGUE, ids=lambda s: s[0])
def test_kernel_form_bits_of_the_catalogue(hostsim, scenes_lib, earth, scene, real_bytes):
    """tests/test_gpu_parity.py::test_kernel_forms_agree, the block after "the timed instantiation (no counters)": bits 2, 3, 4 and 5 per catalogue scene
    under the forced lane-owns-path form and the forced decoupled form, bit 1 only under `plain`, bit 0 under `wave` — and, per plan, that the
    instantiation it names is the one those bits describe."""
    name, param = scene
    sc, _ = util.build(hostsim, scenes_lib, name, earth, param)
    lean = bool(hostsim.lib.hostsim_scene_flags(sc.handle) & 1)
    assert lean == (name in ("cornell_box", "spheres_1m"))
    n_nodes = plan(hostsim, sc, real_bytes).n_nodes
    # (rt_types.hpp lds_form_bytes: seven 16-byte pieces a node record and 16 + 1 stack words for each of the block's 1024 lanes, in a CU's 160 KB)
    fits = n_nodes * 112 + 17 * 1024 * 4 <= LDS_BYTES_PER_CU
    assert fits == (name != "spheres_1m")
    for form in (PLAIN, PLAINGLOBAL, WAVE):
        for count in (0, 1):
            pl = plan(hostsim, sc, real_bytes, count=count, forced=form)
            bits = pl.form_bits
            assert bits < 64 and (bits & 1) == (1 if form == WAVE else 0) == pl.decoupled
            assert (bits & 2) == 0 or form == PLAIN            # bit 1: node records resident in LDS (the lane-owns-path kernel only)
            assert pl.lds == (form == PLAIN and fits) and pl.count == count and pl.list == 0
            assert pl.lds_bytes <= LDS_BYTES_PER_CU and pl.block % 64 == 0 and 64 <= pl.block <= 1024
            assert bits == plan(hostsim, sc, real_bytes, count=1 - count, forced=form).form_bits   # (a counting render reports what its timed twin runs)
    st = plan(hostsim, sc, real_bytes, forced=PLAIN)
    bits = st.form_bits
    assert ((bits & 2) != 0) == fits and st.lds_nodes & 0xFFFFFF == (n_nodes if fits else 0) and st.block == (1024 if fits else 256)
    assert ((bits & 4) != 0) == ((bits & 2) != 0 and st.n_nodes <= 16), (bits, st.n_nodes)
    assert ((bits & 4) != 0) == (name in ("cornell_box", "smoke_cornell_box"))
    assert ((bits & 8) != 0) == ((bits & 2) != 0), bits        # (the LDS form of this kernel has that instantiation)
    assert ((bits & 16) != 0) == (name == "cornell_box"), bits  # (bit 4: ... the one that tests single wrapped records in place)
    assert ((bits & 32) != 0) == ((bits & 8) != 0 and name in ("cornell_box", "spheres_1m")), bits
    assert st.steps == (3 if bits & 4 else 2)
    assert st.shapes == ({0: SHAPES_NONE, 16: SHAPES_SINGLE, 32: SHAPES_NONE_NT, 48: SHAPES_SINGLE_NT}[bits & 48] if bits & 8 else SHAPES_FAST)
    counting = plan(hostsim, sc, real_bytes, count=1, forced=PLAIN)
    assert counting.shapes == SHAPES_FAST and counting.steps == 2       # (the tallied loop: two node steps, the shapes that tally)
    assert counting.key(count=0, shapes=st.shapes, steps=st.steps) == st.key()
    glob = plan(hostsim, sc, real_bytes, forced=PLAINGLOBAL)
    assert glob.form_bits == 0 and glob.block == 256 and glob.lds_nodes == 0 and glob.staged_bytes == 0 and glob.shapes == SHAPES_FAST
    wave = plan(hostsim, sc, real_bytes, forced=WAVE)
    assert ((wave.form_bits & 8) != 0) == (name != "cornell_box"), wave.form_bits   # (cornell_box's two wrapped blocks are instance leaves)
    assert (wave.form_bits & (2 | 4 | 16)) == 0 and ((wave.form_bits & 32) != 0) == (name == "spheres_1m")
    assert wave.shapes == (SHAPES_FAST if name == "cornell_box" else SHAPES_NONE_NT if name == "spheres_1m" else SHAPES_NONE)
    assert wave.quantised == 1 and wave.lds_nodes == 0 and plan(hostsim, sc, real_bytes, count=1, forced=WAVE).shapes == SHAPES_FAST
    # left to itself the plan takes the form by the measured crossover: 5 000 four-wide nodes in f32, 9 000 in f64
    assert plan(hostsim, sc, real_bytes).key() == (wave if n_nodes >= (5000 if real_bytes == 4 else 9000) else st).key()


@pytest.mark.parametrize("real_bytes", [4, 8], ids=["f32", "f64"])
@pytest.mark.parametrize("n_spheres", [60000, 150000])
def test_a_cloud_beyond_the_crossover_selects_the_decoupled_lean_kernel(hostsim, scenes_lib, n_spheres, real_bytes):
    """tests/test_gpu_parity.py::test_decoupled_kernel_is_what_large_scenes_run and test_decoupled_lean_flavour_does_not_depend_on_its_block_size: a
    spheres_1m cloud beyond the measured crossover (5 000 four-wide nodes in f32, 9 000 in f64) selects the decoupled kernel by itself — bit 0 —, the
    instantiation without instance code (bit 3) in its LEAN flavour (bit 5), as ONE block of as many waves as a CU's LDS holds (16 in f32, 13 in
    f64); RTTNW_WAVE_BLOCK changes the block and nothing else."""
    sc, _ = util.build(hostsim, scenes_lib, "spheres_1m", None, n_spheres)
    pl = plan(hostsim, sc, real_bytes)
    assert pl.n_nodes >= 9000, pl.n_nodes                       # (the host builder's tree of this cloud: beyond both crossovers)
    assert pl.form_bits == 1 | 8 | 32 and pl.decoupled and pl.shapes == SHAPES_NONE_NT and pl.quantised
    assert pl.block == 64 * (16 if real_bytes == 4 else 13) and pl.lds_bytes <= LDS_BYTES_PER_CU
    for block, got in ((256, 256), (64, 64), (832, 832), (1024, pl.block), (100, pl.block), (2048, pl.block)):
        other = plan(hostsim, sc, real_bytes, wave_block=block)
        assert other.block == got and other.lds_bytes * pl.block == pl.lds_bytes * got
        assert other.key(block=0, lds_bytes=0) == pl.key(block=0, lds_bytes=0)
    assert plan(hostsim, sc, real_bytes, forced=PLAIN).form_bits & 1 == 0


@pytest.mark.parametrize("scene", CATALOGUE + [("spheres_1m", 60000)], ids=lambda s: "%s_%d" % s)
def test_a_listed_plan_is_the_unlisted_one(hostsim, scenes_lib, earth, scene):
    """The active-list instantiation (rttnw_render_adaptive's refinement passes) is the scene's own kernel over another job numbering: a listed plan
    equals the unlisted one in every field but the list flag, and a counting plan never names a LIST kernel (none tallies)."""
    sc, _ = util.build(hostsim, scenes_lib, scene[0], earth, scene[1])
    for real_bytes in (4, 8):
        for form in (AUTO, PLAIN, PLAINGLOBAL, WAVE):
            plain = plan(hostsim, sc, real_bytes, forced=form)
            listed = plan(hostsim, sc, real_bytes, listed=1, forced=form)
            assert listed.list == 1 and plain.list == 0 and listed.key(list=0) == plain.key()
            counting = plan(hostsim, sc, real_bytes, count=1, listed=1, forced=form)
            assert counting.list == 0 and counting.key() == plan(hostsim, sc, real_bytes, count=1, forced=form).key()
