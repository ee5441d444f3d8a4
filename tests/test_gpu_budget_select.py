"""rttnw_budget_select on the MI355X, held to the numpy restatement of its contract (tests/budget_ref.py) bit for bit: priorities compared as bit
patterns, masks and counts, on the hostile maps of tests/test_budget_cpu.py, on frames of 1x1, 7x5, 61x47, 256x256 (an exact multiple of any
workgroup) and 257x129, for m = 0, 1, candidates - 1, candidates, candidates + 5 and a value inside every tie group — on the two large frames, where
a map holds thousands of groups and each cut is a selection over the whole frame, inside the three groups of highest and the three of lowest
priority (tests/test_budget_cpu.py cuts every group of the same maps' smaller frames).  At 257x129 a map of its own makes
every digit of the radix select decide: priorities over hundreds of exponents, neighbours in the last mantissa bit, and a block of 5000 equal
priorities that m cuts, so that the threshold is found among keys that differ in their index alone."""
import numpy as np
import pytest

import budget_ref
from rttnw_amd import render

pytestmark = pytest.mark.gpu
SIZES = [(1, 1), (7, 5), (61, 47), (256, 256), (257, 129)]
NAMES = list(budget_ref.hostile_maps(1, 1))


def _held_to_the_restatement(args, ms):
    lin, se, spp, cap, rel, ab = args
    for m in ms:
        want_mask, want_rho, want_m = budget_ref.select(lin, se, spp, cap, rel, ab, m)
        mask, rho, got_m, kernel_ms = render.budget_select(lin, se, spp, cap, rel, ab, m, want_ms=True)
        assert (rho.view(np.uint64) == want_rho.view(np.uint64)).all(), m
        assert got_m == want_m == int(mask.sum()), (m, got_m, want_m, int(mask.sum()))
        bad = np.argwhere(mask != want_mask)
        assert bad.size == 0, (m, "the mask differs at (row, col)", bad[:8].tolist())
        assert kernel_ms > 0.0


@pytest.mark.parametrize("w,h", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_device_equals_the_restatement_on_hostile_maps(gpu, w, h):
    for name, args in budget_ref.hostile_maps(w, h).items():
        rho = budget_ref.priority(*args)
        ms = budget_ref.budgets(rho, tie_groups=3 if w * h > 4096 else None)
        try:
            _held_to_the_restatement(args, ms)
        except AssertionError as e:
            raise AssertionError("%s at %dx%d: %s" % (name, w, h, e))


def every_digit_map(w=257, h=129):
    """257x129, value 1, rel_error 1, abs_error 0: the priority of a pixel IS its standard error in r.  Exponents 1 .. 900, pairs that differ in
    the last mantissa bit, 5000 pixels at exactly 7.25 scattered over the frame, 300 pixels without samples (+inf), 500 stopped pixels."""
    rng = np.random.default_rng(11)
    n = w * h
    se_r = 2.0 ** rng.integers(1, 900, n) * (1.0 + rng.random(n))
    order = rng.permutation(n)
    tied, twins, holes, stopped = order[:5000], order[5000:7000], order[7000:7300], order[7300:7800]
    se_r[tied] = 7.25
    se_r[twins[1::2]] = np.nextafter(se_r[twins[0::2]], np.inf)
    se_r[stopped] = 0.5
    spp = np.full(n, 32, np.uint32)
    spp[holes] = 0
    lin = np.ones((h, w, 3))
    se = np.zeros((h, w, 3))
    se[..., 0] = se_r.reshape(h, w)
    return (lin, se, spp.reshape(h, w), 128, 1.0, 0.0), tied


def test_every_digit_decides_at_257x129(gpu):
    args, tied = every_digit_map()
    rho = budget_ref.priority(*args).reshape(-1)
    assert (rho[tied] == 7.25).all() and (rho == 7.25).sum() == 5000 and np.isinf(rho).sum() == 300 and (rho == 0.0).sum() == 500
    assert len(np.unique(np.frexp(rho[np.isfinite(rho) & (rho > 0)])[1])) > 500                      # hundreds of exponents
    above = int((rho > 7.25).sum())
    # cuts through the +inf group, between neighbours in the last bit, and five through the block of equal priorities — among them one key
    # into it, one key short of its end, and its two ends
    n = int((rho > 0).sum())
    ms = [0, 1, 150, 300, 301, 1000, above - 1, above, above + 1, above + 2048, above + 4095, above + 4999, above + 5000, above + 5001,
          n - 1, n, n + 5, 1 << 40]
    _held_to_the_restatement(args, ms)
    mask, _, m = render.budget_select(*args, above + 2048)
    inside = np.flatnonzero(mask.reshape(-1)[np.sort(tied)])
    assert len(inside) == 2048 and (inside == np.arange(2048)).all()                                   # the block's first 2048 pixels in row-major order
