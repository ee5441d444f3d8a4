"""The re-anchored per-bounce tier on the device (tests/util.py compare_paths_reanchored): every bounce of the probe kernel's paths —
f32, contracted f64 and strict f64 — against the f64 oracle's same operation at the probe's own input, and the trace kernels tied
sample by sample to that probe.  The checker itself is checked on the host core in tests/test_bounce_tiers_cpu.py.

Bounds (util.compare_paths_reanchored): K = 8 (perturbations of K eps), w = 32 (eps x scale beyond the oracle's hull).  The budget they
come from, for the f32 kernels: v_rcp_f32 1 ulp, v_sqrt_f32 2.5 ulp, and the sphere test's chain — |d|^2, half_b, the cancellation-free
l = oc - (half_b / a) d, a (r^2 - |l|^2), the square root and the quotient — about 16 roundings of its largest term, the slab / rect
quotients 3; w = 32 is twice the longest chain, K = 8 half of it (a perturbation moves one coordinate, an error all three).
Measured on the MI355X: see each test's docstring (in eps x scale beyond the hull, the largest over every scene and builder).
Evidence that the tier sees what the statistical f32 tests do not: with v_rcp_f32 scaled by (1 + 2^-18) in rt_rcp<float> alone,
test_f32_bounces_equal_oracle_reanchored fails on 11 of its 16 cases (every scene with spheres), while test_T2_f32_vs_oracle[cornell_box]
and test_f32_low_spp_shares_decisions_with_f64 still pass (test_T2_f32_vs_oracle[final_scene] catches it too)."""
import numpy as np
import pytest

import util
from oracle import rto
from rttnw_amd import abi, render

pytestmark = pytest.mark.gpu

SAH, LBVH, DSAH = abi.BVH_HOST_SAH, abi.BVH_DEVICE_LBVH, abi.BVH_DEVICE_SAH
CASES = [("random_scene", 0, SAH), ("two_spheres", 0, SAH), ("two_perlin_spheres", 0, SAH), ("earth", 0, SAH), ("simple_light", 0, SAH),
         ("empty_cornell_box", 0, SAH), ("cornell_box", 0, SAH), ("smoke_cornell_box", 0, SAH), ("final_scene", 0, SAH),
         ("spheres_1m", 20000, SAH), ("cornell_box", 0, LBVH), ("final_scene", 0, LBVH), ("spheres_1m", 20000, LBVH),
         ("cornell_box", 0, DSAH), ("final_scene", 0, DSAH), ("spheres_1m", 20000, DSAH)]
IDS = ["%s-%s" % (c[0], {SAH: "sah", LBVH: "lbvh", DSAH: "dsah"}[c[2]]) for c in CASES]

_oracle_scenes = {}


def _oracle_scene(oracle, scenes_lib, earth, name, param):
    if (name, param) not in _oracle_scenes:
        _oracle_scenes[(name, param)] = util.build(oracle, scenes_lib, name, earth, param,
                                                   bvh=rto.BVH_MEDIAN_SPLIT if name == "spheres_1m" else None)[0]
    return _oracle_scenes[(name, param)]


def _run(gpu, oracle, scenes_lib, earth, case, precision, n_pairs=150, **kw):
    name, param, bvh = case
    sg, setup = util.build(gpu, scenes_lib, name, earth, param, bvh=bvh)
    so = _oracle_scene(oracle, scenes_lib, earth, name, param)
    cam, p = util.params_for(setup, 96, 96, 8, seed=21, precision=precision)
    rng = np.random.default_rng(23)
    pairs = [(int(rng.integers(96)), int(rng.integers(96)), int(rng.integers(8))) for _ in range(n_pairs)]
    res = util.compare_paths_reanchored(lambda x, y, s: util.product_probe_tail(gpu.debug_probe_path, gpu, sg, cam, p, x, y, s), so, cam, p,
                                        pairs, util.EPS_F32 if precision == abi.F32 else util.EPS_F64, **kw)
    print(res.report("%s param %d bvh %d precision %d:" % (name, param, bvh, precision)))
    assert res.paths == n_pairs and res.bounces >= 20   # (spheres_1m at 96 x 96: most camera rays see only sky)
    return res


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_f32_bounces_equal_oracle_reanchored(gpu, oracle, scenes_lib, earth, case):
    """The f32 probe kernel (v_rcp_f32 quotients, the widened f32 slab test, fmed3 box tests, 24-bit uniforms) bounce by bounce against
    the f64 oracle at the kernel's own input: continuous values within the hull of the oracle's 13 evaluations widened by 32 eps x scale,
    decisions the oracle's unless a perturbed evaluation takes the kernel's (at most 2 % of the paths), at every depth, on every catalogue
    scene and every tree builder.  Measured: no flip in 2 400 paths; beyond the hull t 3.98 (final_scene), normal 3.14, scattered
    direction 2.91, camera ray 1.43, attenuation 1.18 (earth's image texture), p 0.49, radiance 0 — against w = 32."""
    _run(gpu, oracle, scenes_lib, earth, case, abi.F32)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_f64_contracted_bounces_reanchored(gpu, oracle, scenes_lib, earth, case):
    """The contracted f64 kernels under the same tier with f64 eps — no growth factor: re-anchored, a last-place difference at bounce 2
    no longer makes bounce 6 another ray (tests/test_gpu_parity.py test_per_bounce_records_equal_oracle keeps the growth-loosened form).
    Measured: no flip; beyond the hull normal 26.2 (spheres_1m: the normal of a small sphere's textbook-discriminant hit), otherwise
    <= 1.23 (camera ray, normal) — against w = 32."""
    _run(gpu, oracle, scenes_lib, earth, case, abi.F64)


@pytest.mark.parametrize("name", ["final_scene", "smoke_cornell_box", "cornell_box", "random_scene"])
def test_f64_strict_bounces_reanchored(gpu, oracle, scenes_lib, earth, name):
    """RTTNW_F64_STRICT: the reference's operations in its order, so the strict form of the checker — no perturbation, no flip —
    finds nothing beyond 1e-12 of the oracle at the kernel's input, at any bounce.  Measured: largest relative difference 2.5e-16
    (final_scene p, t, uv), no flip."""
    res = _run(gpu, oracle, scenes_lib, earth, (name, 0, SAH), abi.F64_STRICT, strict_tol=1e-12, max_flip_share=0.0)
    assert not res.flips and max(res.excess.values()) <= 1e-12


FORMS = [("cornell_box", 0, "plain"), ("cornell_box", 0, "plainglobal"), ("cornell_box", 0, "wave"),
         ("final_scene", 0, "plain"), ("final_scene", 0, "plainglobal"), ("final_scene", 0, "wave"), ("spheres_1m", 70000, None)]


@pytest.mark.parametrize("precision", [abi.F32, abi.F64], ids=["f32", "f64"])
def test_trace_kernels_equal_the_probe_per_sample(gpu, oracle, scenes_lib, earth, precision, monkeypatch):
    """The probe (probe_path_kernel) is a kernel of its own: a miscompile of one trace kernel (ROCm's SLP vectoriser once made
    trace_kernel<float> return 0 for ~0.5 % of the paths that end on a light) would not show in it.  So the trace kernels are tied to
    the probe the tiers above validate: spp 1 frames on a black background, sample_begin 0 and 5 — a pixel's linear value is then that
    one sample's radiance — against the probe's tail for (px, row, sample_begin) on 512 fixed pixels, in every kernel form (RTTNW_KERNEL
    plain, plainglobal, wave on cornell_box and final_scene; the decoupled kernel over the interleaved buffer, stats.reserved bits 0 and
    6, on spheres_1m at 70 000).  f32: within 64 * 2^-24 relative on >= 99.8 % of the pixels (two compilations of the same steps may fuse
    a multiply-add differently); f64: within 1e-12 relative.  Beyond that only a pixel whose path the checker calls an allowed flip may
    differ grossly (zero in one, above 1e-3 in the other).  Measured: no pixel outside the bound in either precision, any form."""
    W = H = 64
    rng = np.random.default_rng(29)
    idx = rng.choice(W * H, 512, replace=False)
    rows, cols = idx // W, idx % W
    eps = util.EPS_F32 if precision == abi.F32 else util.EPS_F64
    scenes, tails = {}, {}
    for name, param, form in FORMS:
        if name not in scenes:
            sg, setup = util.build(gpu, scenes_lib, name, earth, param)
            scenes[name] = (sg, setup)
        sg, setup = scenes[name]
        for sb in (0, 5):
            cam, p = util.params_for(setup, W, H, 1, seed=21, precision=precision, sample_begin=sb)
            p.background = abi.vec3(0.0, 0.0, 0.0)
            if (name, sb) not in tails:
                pp = util.params_for(setup, W, H, 1, seed=21, precision=precision)[1]
                pp.background = abi.vec3(0.0, 0.0, 0.0)
                tails[(name, sb)] = np.array([util.product_probe_tail(gpu.debug_probe_path, gpu, sg, cam, pp, int(x), int(y), sb)[1][0:3]
                                              for x, y in zip(cols, rows)])
            if form is None:
                monkeypatch.delenv("RTTNW_KERNEL", raising=False)
            else:
                monkeypatch.setenv("RTTNW_KERNEL", form)
            lin, _, st = render.render_host(sg, cam, p)
            if form is None:
                assert (st.reserved & 65) == 65, st.reserved
            got, ref = lin[rows, cols], tails[(name, sb)]
            rel = (np.abs(got - ref) / np.maximum(np.maximum(np.abs(got), np.abs(ref)), 1e-300)).max(axis=1)
            bound = 64 * eps if precision == abi.F32 else 1e-12
            out = np.nonzero(rel > bound)[0]
            for i in out:
                print("%s %s sample %d px %d row %d: kernel %s probe %s" % (name, form, sb, cols[i], rows[i], got[i], ref[i]))
            if precision == abi.F32:
                assert len(out) <= 0.002 * len(idx), (name, form, sb, len(out))
            gross = [i for i in out if (got[i].max() == 0.0 and ref[i].max() > 1e-3) or (ref[i].max() == 0.0 and got[i].max() > 1e-3)]
            if precision != abi.F32:
                gross = list(out)
            if gross:
                so = _oracle_scene(oracle, scenes_lib, earth, name, param)
                pp = util.params_for(setup, W, H, 1, seed=21, precision=precision)[1]
                for i in gross:
                    res = util.compare_paths_reanchored(
                        lambda x, y, s: util.product_probe_tail(gpu.debug_probe_path, gpu, sg, cam, pp, x, y, s), so, cam, pp,
                        [(int(cols[i]), int(rows[i]), sb)], eps, max_flip_share=1.0)
                    assert res.flips, (name, form, sb, cols[i], rows[i], got[i], ref[i])
    monkeypatch.delenv("RTTNW_KERNEL", raising=False)
