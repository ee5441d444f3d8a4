"""What the tests of rttnw_temporal_probe share (tests/test_probe_cpu.py on the host harness, tests/test_gpu_probe.py on the device): the chains of
frames both are held to and the checks of the properties both must have.  An implementation under test is a function
run(features, cam, history=None, boost=..., fill=..., **parameters) -> dict of probe_ref.OUTPUTS.  The probe keeps no colour, so the history of
the next link is rttnw_temporal_accumulate's restated (temporal_ref.accumulate) over the same frame — which is also what the contract's stated
consequence is held against."""
import numpy as np

import probe_ref
import temporal_ref
import variance_cases
from temporal_cases import SIZES, same

BOOSTS, FILLS, MAX_HISTORY = (1, 2, 4, 8), (1.0, 3.5, 8.0, 100.0), (1, 4, 32)
# (size, boost, fill, max_history, normal_min, depths from the analytic scene, non-finite values): every size with every boost and every fill; the
# other settings alternate as in the siblings' grids, so that each meets every size, boost and fill; a quarter of the cases carry NaN and inf in
# depth and length
CASES = [(size, b, fl, MAX_HISTORY[(i + j + k) % 3], (-1.0, 0.0)[(i + k) % 2], (j + k) % 2 == 0, (3 * i + j + k) % 4 == 0)
         for i, size in enumerate(SIZES) for j, b in enumerate(BOOSTS) for k, fl in enumerate(FILLS)]
CASE_IDS = ["%dx%d-b%d-f%g-h%d-%s-%s%s" % (s[0], s[1], b, fl, mh, "no-normal-test" if nm == -1.0 else "normal-test", "analytic" if an else "random",
                                           "-nonfinite" if bad else "") for s, b, fl, mh, nm, an, bad in CASES]
STAIRS = ((0.0, 8), (0.99, 4), (1.0, 4), (3.0, 2), (3.0001, 1), (7.0, 1), (1e9, 1))     # Lp -> m at fill 8, boost 8


def assert_same_outputs(got, want, what=()):
    for name in probe_ref.OUTPUTS:
        assert same(got[name], want[name]), (name,) + tuple(what)


def case_parameters(case):
    return dict(boost=case[1], fill=case[2], max_history=case[3], normal_min=case[4])


def _poison(rng, a, count=5):
    flat = a.reshape(-1)
    where = rng.choice(flat.size, size=min(count, flat.size), replace=False)
    flat[where] = rng.choice([np.nan, np.inf], size=where.size)


def chain(case):
    """(history, [(linear, features, cam)] * 3) of a case: variance_cases.chain of the case's size and settings — a made-up history under one
    camera, then the camera moved, moved again, then bitwise equal — with, in a quarter of the cases, NaN and inf in the history's length and in
    every frame's depth (the history's own included)."""
    size, boost, fill, mh, nm, analytic, bad = case
    history, frames = variance_cases.chain((size, 1 + BOOSTS.index(boost) % 3, mh, 2, nm, analytic, False))
    history = dict(history, variance=None)
    if bad:
        rng = np.random.default_rng(size[0] * 1000 + size[1] * 10 + boost * 100 + int(fill))
        history["length"] = history["length"].copy()
        _poison(rng, history["length"])
        seen = set()
        for f in [history["features"]] + [f for _, f, _ in frames]:
            if id(f) not in seen:                 # (the third and the fourth frame share their features)
                seen.add(id(f))
                f["depth"] = f["depth"].copy()
                _poison(rng, f["depth"])
    return history, frames


def check_link(got, want, stage_a, f, history, kw):
    """One link: every output equals the restatement's, and the stated consequence holds against rttnw_temporal_accumulate restated."""
    assert_same_outputs(got, want)
    m, hit = want["multiplier"], np.asarray(f["alpha"]) != 0.0
    assert np.all(np.isin(m, (1, 2, 4, 8))) and np.all(m <= kw["boost"]) and np.all(m[~hit] == 1)
    assert np.all(want["length"][~hit] == 0.0)
    if kw["boost"] == 1:
        assert np.all(m == 1)
    assert same(probe_ref.grown(want["length"], kw["max_history"]), stage_a["length"]), "the consequence: out_length"
    assert same(want["prev_xy"], stage_a["prev_xy"]), "the consequence: out_prev_xy"
    return int((hit & (m == 1)).sum()), int((hit & (m > 1)).sum())


def check_chain(run, case):
    """Every output of every link equals the restatement's bit for bit, and the probe's length and motion vectors are rttnw_temporal_accumulate's
    (restated) by the stated consequence.  Returns the tallies of the two moved-camera links: hit pixels with m == 1, with m > 1."""
    kw = case_parameters(case)
    ta = {k: kw[k] for k in ("max_history", "normal_min")}
    history, frames = chain(case)
    plain = boosted = 0
    for k, (lin, f, cam) in enumerate(frames):
        want = probe_ref.probe(f, cam, history=history, **kw)
        stage_a = temporal_ref.accumulate(lin, f, cam, history=history, **ta)
        ones, more = check_link(run(f, cam, history=history, **kw), want, stage_a, f, history, kw)
        if k < 2:
            plain, boosted = plain + ones, boosted + more
        history = stage_a
    return plain, boosted


def check_staircase(run):
    """Hand-made lengths under a static camera and flat features: the history's length comes back as Lp, and the multiplier follows the contract's
    staircase at fill 8, boost 8; boost 1 gives all ones; a miss gets 1 whatever its history."""
    from temporal_cases import cameras
    from variance_cases import flat_features
    w, h = len(STAIRS), 3
    cam = cameras(w / h)[0]
    prev_cam = type(cam).from_buffer_copy(cam)
    f = flat_features(w, h)
    f["alpha"][2, :] = 0.0                                                  # the bottom row misses
    f["depth"][2, :] = 0.0
    length = np.tile(np.array([lp for lp, _ in STAIRS]), (h, 1))
    history = {"length": length, "features": flat_features(w, h), "cam": prev_cam}
    got = run(f, cam, history=history, boost=8, fill=8.0)
    assert same(got["length"][:2], length[:2]) and np.all(got["length"][2] == 0.0)
    assert got["multiplier"][:2].tolist() == [[m for _, m in STAIRS]] * 2, got["multiplier"].tolist()
    assert np.all(got["multiplier"][2] == 1)
    assert same(run(f, cam, history=history)["multiplier"], got["multiplier"])          # a 0 is the default: boost 8, fill 8.0
    assert np.all(run(f, cam, history=history, boost=1, fill=100.0)["multiplier"] == 1)
    assert run(f, cam, history=history, boost=4, fill=8.0)["multiplier"][0].tolist() == [4, 4, 4, 2, 1, 1, 1]
    first = run(f, cam, boost=8, fill=3.5)                                   # no history: min(boost, largest power of two <= floor(fill))
    assert np.all(first["length"] == 0.0) and np.isnan(first["prev_xy"]).all()
    assert np.all(first["multiplier"][:2] == 2) and np.all(first["multiplier"][2] == 1)
