"""rttnw_temporal_probe without a GPU: the host build of the arithmetic the device kernel runs (rttnw_amd/csrc/probe.hpp, built by
tests/probe_host) against a numpy restatement of the contract in include/rttnw_hip.h — bit for bit, every output, along chains of three calls —,
the multiplier's staircase on hand-made lengths, and the contract's stated consequence: the probe's length and motion vectors against
rttnw_temporal_accumulate's restatement (tests/temporal_ref.py) and its host build (tests/temporal_host)."""
import numpy as np
import pytest

import probe_ref
import temporal_ref
from temporal_cases import same
from probe_cases import BOOSTS, CASE_IDS, CASES, FILLS, STAIRS, case_parameters, chain, check_chain, check_staircase


@pytest.fixture(scope="module")
def host():
    return probe_ref.host()


def test_the_cases_are_the_stated_matrix():
    assert len(CASES) == 64 and len(set(CASE_IDS)) == 64
    assert sum(1 for c in CASES if c[6]) == 16                             # a quarter carry NaN and inf
    for size in {c[0] for c in CASES}:
        assert {(c[1], c[2]) for c in CASES if c[0] == size} == {(b, f) for b in BOOSTS for f in FILLS}
    assert {c[3] for c in CASES} == {1, 4, 32} and {c[4] for c in CASES} == {-1.0, 0.0} and {c[5] for c in CASES} == {True, False}
    bad = [c for c in CASES if c[6]]
    history, frames = chain(bad[-1])
    assert not np.isfinite(history["length"]).all() and all(not np.isfinite(f["depth"]).all() for _, f, _ in frames)


def test_the_restatement_alone_meets_the_cases_condition():
    """Over the moved-camera links of the cases, by the numpy restatement alone: hit pixels with m == 1 and hit pixels with m > 1 both occur — in
    all, and within every case of at least 37x29 whose boost and fill leave both open (boost > 1, fill 3.5 or 8) and whose depths are the analytic
    scene's (so that taps are accepted)."""
    plain = boosted = 0
    for case in CASES:
        ones, more = check_chain(probe_ref.probe, case)
        plain, boosted = plain + ones, boosted + more
        if case[1] == 1 or case[2] == 1.0:
            assert more == 0, case
        elif case[0][0] >= 37 and case[5] and case[2] in (3.5, 8.0):
            assert ones > 0 and more > 0, (case, ones, more)
    print("hit pixels of the moved-camera links: %d with m == 1, %d with m > 1" % (plain, boosted))
    assert plain > 0 and boosted > 0


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_host_build_equals_the_numpy_restatement_bit_for_bit(host, case):
    """... and, link by link, the stated consequence against temporal_ref.accumulate: out_length is Lp == 0 ? 1 : min(Lp + 1, max_history) and the
    two out_prev_xy are equal bitwise, NaNs included."""
    print("hit pixels with m == 1: %d, with m > 1: %d" % check_chain(host, case))


def test_the_consequence_holds_against_the_host_build_of_temporal_accumulate(host):
    """The two host builds against each other: probe.hpp calls what temporal.hpp calls."""
    accumulate = temporal_ref.host()
    for case in (c for c in CASES if c[0] == (70, 41)):
        kw = case_parameters(case)
        ta = {k: kw[k] for k in ("max_history", "normal_min")}
        history, frames = chain(case)
        for lin, f, cam in frames:
            got, nxt = host(f, cam, history=history, **kw), accumulate(lin, f, cam, history=history, **ta)
            assert same(probe_ref.grown(got["length"], kw["max_history"]), nxt["length"]) and same(got["prev_xy"], nxt["prev_xy"]), case
            history = nxt


def test_the_multiplier_staircase(host):
    check_staircase(host)
    check_staircase(probe_ref.probe)
    lengths = np.array([lp for lp, _ in STAIRS])
    assert probe_ref.multiplier(lengths, True, 8, 8.0).tolist() == [m for _, m in STAIRS]
    assert probe_ref.multiplier(np.array([np.nan, np.inf]), True, 8, 8.0).tolist() == [1, 1]   # a NaN compares false; 8 / inf = 0


def test_zero_parameters_are_the_stated_defaults(host):
    history, frames = chain(CASES[-6])
    _, f, cam = frames[0]
    default = host(f, cam, history=history)
    for name in probe_ref.OUTPUTS:
        assert same(default[name], host(f, cam, history=history, boost=8, fill=8.0, max_history=32, depth_tolerance=0.05, normal_min=0.9)[name]), name
    assert not np.array_equal(default["multiplier"], host(f, cam, history=history, boost=2)["multiplier"])
    assert not np.array_equal(default["multiplier"], host(f, cam, history=history, fill=2.0)["multiplier"])


def test_no_history_is_the_first_frames_rule(host):
    _, frames = chain(CASES[-6])
    _, f, cam = frames[0]
    hit = np.asarray(f["alpha"]) != 0.0
    assert hit.any() and not hit.all()
    for run in (host, probe_ref.probe):
        for boost, fill, want in ((8, 8.0, 8), (8, 100.0, 8), (4, 100.0, 4), (8, 3.5, 2), (8, 1.0, 1), (1, 8.0, 1), (2, 7.99, 2), (8, 7.99, 4)):
            first = run(f, cam, boost=boost, fill=fill)
            assert np.all(first["length"] == 0.0) and np.isnan(first["prev_xy"]).all()
            assert np.all(first["multiplier"][hit] == want) and np.all(first["multiplier"][~hit] == 1), (boost, fill)
