"""rttnw_denoise_nlm without a GPU: the host build of the arithmetic the device kernels run (rttnw_amd/csrc/nlm.hpp, built by tests/nlm_host)
against a numpy restatement of the contract in include/rttnw_hip.h — bit for bit — and the properties the contract promises: the exchange of
the two halves, locality, the weight of the centre, non-finite values that propagate."""
import numpy as np
import pytest

import nlm_ref
from nlm_cases import FRAMES, KS, RADII, crop_interior, same_bits, swapped_equal


@pytest.fixture(scope="module")
def host():
    return nlm_ref.host()


@pytest.mark.parametrize("with_variance", [True, False], ids=["variance", "pair-variance"])
@pytest.mark.parametrize("radii", RADII, ids=lambda rf: "r%d-f%d" % rf)
@pytest.mark.parametrize("size", FRAMES, ids=lambda s: "%dx%d" % s)
def test_host_build_equals_the_numpy_restatement_bit_for_bit(host, size, radii, with_variance):
    rng = np.random.default_rng(size[0] * 64 + radii[0] * 2 + int(with_variance))
    a, b, va, vb = nlm_ref.random_inputs(rng, size[0], size[1], with_variance)
    for k in KS:
        got = host(a, b, va, vb, radii[0], radii[1], k)
        want = nlm_ref.denoise_nlm(a, b, va, vb, radii[0], radii[1], k)
        for name in nlm_ref.OUTPUTS:
            assert same_bits(got[name], want[name]), (name, k, np.nanmax(np.abs(got[name].astype(np.float64) - want[name])))
    if size != (1, 1):
        assert not np.array_equal(got["linear"], (a + b) * 0.5)        # ... and it did filter something


def test_zero_parameters_are_the_stated_defaults(host):
    rng = np.random.default_rng(11)
    a, b, va, vb = nlm_ref.random_inputs(rng, 21, 19)
    assert same_bits(host(a, b, va, vb)["linear"], host(a, b, va, vb, 7, 3, 0.7)["linear"])
    assert not same_bits(host(a, b, va, vb)["linear"], host(a, b, va, vb, 7, 3, 0.45)["linear"])


@pytest.mark.parametrize("with_variance", [True, False], ids=["variance", "pair-variance"])
def test_exchanging_the_halves_exchanges_the_filtered_halves_only(host, with_variance):
    rng = np.random.default_rng(3)
    a, b, va, vb = nlm_ref.random_inputs(rng, 37, 29, with_variance)
    swapped_equal(host(a, b, va, vb), host(b, a, vb, va))


@pytest.mark.parametrize("radii", [(7, 3), (2, 4), (16, 4)], ids=lambda rf: "r%d-f%d" % rf)
def test_a_pixel_depends_on_r_plus_f_plus_1_pixels_around_it(host, radii):
    """The interior of a crop taken with a margin of r + f + 1 equals the same pixels of the whole frame's result: a halo one pixel short, or a
    clamp applied where the image does not end, shows here."""
    r, f = radii
    rng = np.random.default_rng(r)
    m = r + f + 1
    w, h = 2 * m + 9, 2 * m + 6
    for with_variance in (True, False):
        a, b, va, vb = nlm_ref.random_inputs(rng, w + 13, h + 11, with_variance)
        whole = host(a, b, va, vb, r, f)
        crop = (slice(4, 4 + h), slice(6, 6 + w))
        part = host(a[crop], b[crop], None if va is None else va[crop], None if vb is None else vb[crop], r, f)
        for name in nlm_ref.OUTPUTS:
            assert same_bits(crop_interior(part[name], m), crop_interior(whole[name][crop], m)), (name, with_variance)
        # ... and the margin is not generous: one pixel further out the crop's edge is felt (the guides reach r + f pixels, the pair
        # variance's 3x3 one more; a given variance is read as it is)
        short = m - 1 if va is None else m - 2
        assert not same_bits(crop_interior(part["linear"], short), crop_interior(whole["linear"][crop], short))


def test_equal_halves_without_noise_average_freely_and_an_edge_stops_them(host):
    """Two identical halves have a pair variance of 0: across a step of 0.5 the distance is 0.25 / 1e-10 and the weight vanishes; inside a flat
    region every weight is 1 and the value stays."""
    h, w = 24, 30
    img = np.zeros((h, w, 3))
    img[:, : w // 2] = [0.2, 0.3, 0.4]
    img[:, w // 2:] = [0.7, 0.8, 0.9]
    out = host(img, img, None, None, 5, 2)
    assert np.all(np.abs(out["linear"] - img) <= 1e-12)
    assert np.all(out["error"] == 0.0)


def test_non_finite_values_propagate_and_stay_local(host):
    rng = np.random.default_rng(5)
    r, f = 3, 2
    a, b, va, vb = nlm_ref.random_inputs(rng, 40, 33)
    clean = host(a, b, va, vb, r, f)
    bad = a.copy()
    bad[16, 20, 1] = np.nan
    out = host(bad, b, va, vb, r, f)
    assert np.isnan(out["linear"][16, 20]).any()                      # the centre weighs 1: its own value always enters
    far = np.ones((33, 40), dtype=bool)
    far[16 - (r + f):16 + r + f + 1, 20 - (r + f):20 + r + f + 1] = False
    assert same_bits(out["linear"][far], clean["linear"][far]) and np.isfinite(out["linear"][far]).all()
    # a NaN variance makes NaN distances, and those NaN weights: nothing maps it to a number
    bad_v = vb.copy()
    bad_v[16, 20] = np.nan
    out = host(a, b, va, bad_v, r, f)
    assert np.isnan(out["half_a"][16, 20]).all() and same_bits(out["half_b"], clean["half_b"])
    assert same_bits(out["linear"][far], clean["linear"][far])
