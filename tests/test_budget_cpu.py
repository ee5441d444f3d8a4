"""The arithmetic of rttnw_budget_select without a GPU: the host build of rttnw_amd/csrc/budget_select.hpp (tests/budget_host, a plain sort as its
select) equals the numpy restatement written from the header's contract (tests/budget_ref.py) — priorities compared as bit patterns, masks and
counts — on frames of 1x1, 7x5 and 61x47 pixels, for m = 0, 1, candidates - 1, candidates, candidates + 5 and a value inside every tie group, on
hostile maps; and the radix select's view of a key (digits, prefixes) is held to the key.  (tests/test_gpu_budget_select.py holds the device to
the same restatement.)"""
import numpy as np
import pytest

import budget_ref

SIZES = [(1, 1), (7, 5), (61, 47)]
NAMES = list(budget_ref.hostile_maps(1, 1))


@pytest.fixture(scope="module")
def host():
    return budget_ref.host()


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", NAMES)
def test_host_build_equals_the_restatement(host, name, w, h):
    lin, se, spp, cap, rel, ab = budget_ref.hostile_maps(w, h)[name]
    _, rho, _ = budget_ref.select(lin, se, spp, cap, rel, ab, 0)
    n_cand = int((rho > 0.0).sum())
    for m in budget_ref.budgets(rho):
        want_mask, want_rho, want_m = budget_ref.select(lin, se, spp, cap, rel, ab, m)
        mask, got_rho, got_m = host(lin, se, spp, cap, rel, ab, m)
        assert (got_rho.view(np.uint64) == want_rho.view(np.uint64)).all(), (name, m)
        assert got_m == want_m == min(m, n_cand) == int(mask.sum()), (name, m)
        assert (mask == want_mask).all(), (name, m)
        assert not mask[rho == 0.0].any()                                  # a non-candidate is never selected


def test_the_maps_are_what_their_names_say():
    maps = budget_ref.hostile_maps(61, 47)
    rho = {k: budget_ref.priority(*v) for k, v in maps.items()}
    n = 61 * 47
    assert 0 < (rho["mixed"] > 0).sum() < n and ((rho["mixed"] > 1.0) | (rho["mixed"] == 0.0)).all()
    assert len(np.unique(rho["all equal"])) == 1 and np.isfinite(rho["all equal"]).all() and (rho["all equal"] > 1.0).all()
    assert np.isinf(rho["all inf"]).all()
    assert (rho["no candidate"] == 0.0).all()
    lb = np.unique(rho["last bit"])
    assert len(lb) == 3 and (np.diff(lb.view(np.uint64)) == 1).all()
    v0 = maps["value 0, abs 0"][0]
    assert np.isinf(rho["value 0, abs 0"][(v0 == 0.0).all(axis=-1)]).all() and np.isfinite(rho["value 0, abs 0"]).any()
    sub = rho["subnormal abs"]
    assert np.isinf(sub).any() and (np.isfinite(sub) & (sub > 1.0)).any() and (sub[np.isfinite(sub)] == np.floor(sub[np.isfinite(sub)])).all()
    se_inf = np.isinf(maps["se inf"][1]).any(axis=-1)
    assert se_inf.any() and np.isinf(rho["se inf"][se_inf]).all() and (maps["se inf"][2] > 0).all()
    capped = maps["at the cap, huge error"][2] == 128
    assert capped.any() and (rho["at the cap, huge error"][capped] == 0.0).all()
    holes = maps["NaN where spp is 0"][2] == 0
    assert holes.any() and np.isinf(rho["NaN where spp is 0"][holes]).all() and not np.isnan(rho["NaN where spp is 0"]).any()


def test_order_is_priority_descending_then_index_ascending():
    lin = np.full((2, 3, 3), 1.0)
    se = np.zeros((2, 3, 3))
    se[..., 1] = np.array([[0.5, 0.2, 0.5], [0.9, 0.5, 0.05]])            # rel 0.1: priorities 5, 2, 5, 9, 5 and a stopped pixel
    spp = np.full((2, 3), 16, np.uint32)
    for m, want in [(1, [3]), (2, [3, 0]), (3, [3, 0, 2]), (4, [3, 0, 2, 4]), (5, [3, 0, 2, 4, 1]), (6, [3, 0, 2, 4, 1])]:
        mask, rho, got = budget_ref.select(lin, se, spp, 64, 0.1, 0.0, m)
        assert sorted(np.flatnonzero(mask)) == sorted(want) and got == len(want)
    assert rho[1, 2] == 0.0 and rho[1, 0] == 0.9 / 0.1


def test_the_digits_of_a_key_are_the_key(host):
    rng = np.random.default_rng(5)
    keys = [(0x3FF0000000000001, 0xFFFFFFFF), (0x7FF0000000000000, 0), (0x7FF0000000000000, 0xFFFFFFFF), (0x4000000000000000, 0x00000FFF),
            (0x3FFFFFFFFFFFFFFF, 0xFF000000), (0x400FFFFFFFFFFFF0, 0x00FFF000)]
    keys += [(int(hi), int(lo)) for hi, lo in zip(rng.integers(0x3FF0000000000001, 0x7FF0000000000000, 40), rng.integers(0, 1 << 32, 40))]
    for hi, lo in keys:
        assert host.digits_roundtrip(hi, lo) == 0, (hex(hi), hex(lo))
