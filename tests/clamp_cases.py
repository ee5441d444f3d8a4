"""What the tests of rttnw_temporal_clamp share (tests/test_clamp_cpu.py on the host harness, tests/test_gpu_clamp.py on the device): the chains of
frames both are held to and the checks of the properties both must have.  An implementation under test is a function
run(linear, features, cam, history=None, gamma=..., clamp_radius=..., **parameters) -> dict of clamp_ref.OUTPUTS plus "features" and "cam", so that
a result is the next call's history."""
import numpy as np

import clamp_ref
import variance_cases
import variance_ref
from temporal_cases import SIZES, cameras, same
from variance_cases import flat_features, noisy_frames

RADII, GAMMAS, MAX_HISTORY, MIN_TEMPORAL = (1, 3, 4), (0.25, 1.0, float("inf")), (1, 4, 32), (2, 4)
# (size, radius, gamma, max_history, min_temporal, normal_min, depths from the analytic scene, non-finite values): every size with every radius and
# every gamma; the other settings alternate as in variance_cases.CASES, so that each meets every size, radius and gamma; a quarter of the cases
# carry NaN and inf
CASES = [(size, r, g, MAX_HISTORY[(i + j + k) % 3], MIN_TEMPORAL[(i + j + k) % 2], (-1.0, 0.0)[(i + k) % 2], (j + k) % 2 == 0, (3 * i + j + k) % 4 == 0)
         for i, size in enumerate(SIZES) for j, r in enumerate(RADII) for k, g in enumerate(GAMMAS)]
CASE_IDS = ["%dx%d-r%d-g%s-h%d-t%d-%s-%s%s" % (s[0], s[1], r, g, mh, mt, "no-normal-test" if nm == -1.0 else "normal-test",
                                               "analytic" if an else "random", "-nonfinite" if bad else "") for s, r, g, mh, mt, nm, an, bad in CASES]


def assert_same_outputs(got, want, what=(), names=clamp_ref.OUTPUTS):
    for name in names:
        assert same(got[name], want[name]), (name,) + tuple(what)


def case_parameters(case):
    """The clip's window has the case's radius and so has stage B's."""
    return dict(clamp_radius=case[1], gamma=case[2], max_history=case[3], min_temporal=case[4], normal_min=case[5], radius=case[1])


def chain(case):
    """variance_cases.chain of the case's size and settings: (history, three frames) — the camera moved, moved again, then bitwise equal."""
    size, r, g, mh, mt, nm, analytic, bad = case
    return variance_cases.chain((size, r, mh, mt, nm, analytic, bad))


def check_chain(run, case):
    """Every output of every link equals the restatement's bit for bit — both chains run on their own results.  The restatement alone is tallied:
    with a finite gamma, on a frame of at least 37x29, some channel is clipped and some pixel with a history is left unclipped; with gamma = +inf
    nothing is clipped and the shared outputs are rttnw_temporal_variance's restated (variance_ref.estimate)."""
    kw = case_parameters(case)
    vkw = {k: kw[k] for k in ("max_history", "min_temporal", "normal_min", "radius")}
    got, (want, frames) = chain(case)[0], chain(case)
    clipped = unclipped = 0
    for k, (lin, f, cam) in enumerate(frames):
        nxt = run(lin, f, cam, history=got, **kw)
        prev, want = want, clamp_ref.clamp(lin, f, cam, history=want, **kw)
        assert_same_outputs(nxt, want, (k,))
        bits = want["clipped"]
        assert np.all(bits[np.asarray(f["alpha"]) == 0.0] == 0) and np.all(bits <= 7)
        clipped += int(np.unpackbits(bits[..., None], axis=-1).sum())
        unclipped += int((want["blended"] & (bits == 0)).sum())     # blended: some tap of the history was accepted, W > 0
        plain = variance_ref.estimate(lin, f, cam, history=prev, **vkw)      # rttnw_temporal_variance restated, over the same history
        for name in ("linear", "rgba8", "moment2", "length", "prev_xy"):    # where no channel of a pixel is clipped: its bits
            assert same(want[name][bits == 0], plain[name][bits == 0]), (name, k, "unclipped pixels against variance_ref")
        assert same(want["length"], plain["length"]) and same(want["prev_xy"], plain["prev_xy"]), k
        if np.isinf(kw["gamma"]):
            assert not bits.any(), k
            assert_same_outputs(want, plain, (k, "against variance_ref"), clamp_ref.SHARED)
        got = nxt
    if np.isfinite(kw["gamma"]) and case[0][0] >= 37 and case[0][1] >= 29:
        assert clipped > 0, "the case clips nothing"
        assert unclipped > 0, "the case leaves no pixel with a history unclipped"
    return clipped, unclipped


# ---- properties on made-up frames

def _static(w, h):
    cam = cameras(w / h)[0]
    return cam, type(cam).from_buffer_copy(cam)                       # two descriptors, bitwise equal


def check_a_ghost_goes(run, unclamped):
    """A history with a bright stripe the frame does not have: the clip takes it out in one frame, where rttnw_temporal_variance (`unclamped`)
    keeps 7/8 of it."""
    w, h = 37, 29
    cam, prev_cam = _static(w, h)
    f = flat_features(w, h)
    ghost = np.full((h, w, 3), 0.2)
    ghost[:, 10:15] = 5.0
    history = {"linear": ghost, "moment2": ghost * ghost, "length": np.full((h, w), 8.0), "features": f, "cam": prev_cam}
    lin = np.full((h, w, 3), 0.2)
    got = run(lin, f, cam, history=history, gamma=1.0)
    assert np.all(got["length"] == 9.0)
    assert np.abs(got["linear"] - 0.2).max() <= 1e-6, np.abs(got["linear"] - 0.2).max()
    assert np.all(got["clipped"][:, 10:15] == 7)
    assert (got["moment2"] - got["linear"] * got["linear"]).max() < 1e-6
    plain = unclamped(lin, f, cam, history=history)
    assert plain["linear"][:, 10:15].min() > 4.0, plain["linear"][:, 10:15].min()


def check_noise_stays(run):
    """Eight frames of plain noise under a static camera, radius 3, gamma 3: the clip leaves an honest history alone — at most 2 % of the channels
    are clipped in the second frame and 0.2 % in each later one — and the temporal branch stays unbiased: variance * 8 / sigma^2 within 10 % of 1 in
    each half.  (frames, shares, ratios) are returned for printing."""
    frames, sigma = noisy_frames(8)
    h, w = frames[0].shape[:2]
    cam, f = cameras(w / h)[0], flat_features(w, h)
    history, shares = None, []
    for k, lin in enumerate(frames):
        history = run(lin, f, cam, history=history, gamma=3.0, clamp_radius=3, max_history=32)
        bits = history["clipped"]
        shares.append(float(np.unpackbits(bits[..., None], axis=-1).sum()) / (h * w * 3))
        if k == 0:
            assert shares[0] == 0.0
    assert shares[1] <= 0.02 and all(s <= 0.002 for s in shares[2:]), shares
    assert np.all(history["length"] == 8.0)
    ratios = []
    for half, s in ((slice(0, w // 2), 0.1), (slice(w // 2, w), 0.3)):
        ratios.append(float((history["variance"][:, half] * 8.0).mean() / s ** 2))
        assert abs(ratios[-1] - 1.0) < 0.1, ratios
    return shares, ratios


def check_the_window_respects_edges(run):
    """variance_cases.check_window_respects_edges' two noise-free halves with perpendicular normals: no deviation anywhere, and a history of the
    other half's colour is clipped to the pixel's own half."""
    w = h = 32
    cam, prev_cam = _static(w, h)
    f = flat_features(w, h)
    f["normal"][:, w // 2:] = (1.0, 0.0, 0.0)
    lin = np.full((h, w, 3), 0.2)
    lin[:, w // 2:] = 0.8
    first = run(lin, f, cam, clamp_radius=3)
    assert np.all(first["sd"] <= 1e-7), first["sd"].max()
    assert np.abs(first["mean"] - lin).max() <= 1e-12 and not first["clipped"].any()
    other = np.full((h, w, 3), 0.8)
    other[:, w // 2:] = 0.2
    history = {"linear": other, "moment2": other * other, "length": np.full((h, w), 8.0), "features": f, "cam": prev_cam}
    got = run(lin, f, cam, history=history, clamp_radius=3, gamma=1.0)
    assert np.all(got["clipped"] == 7) and np.all(got["length"] == 9.0)
    assert np.abs(got["linear"] - lin).max() <= 1e-6, np.abs(got["linear"] - lin).max()


def check_miss_pixels(run):
    """alpha == 0 passes through — mean = cur, sd = 0, clipped = 0, also beside a history —, and a miss contributes to no neighbour's window: its
    colour, however wild, changes no other pixel's bounds."""
    rng = np.random.default_rng(5)
    w, h = 37, 29
    cam, prev_cam = _static(w, h)
    f = flat_features(w, h)
    miss = rng.random((h, w)) < 0.2
    f["alpha"][miss] = 0.0
    lin = 0.5 + 0.1 * rng.standard_normal((h, w, 3))
    got = run(lin, f, cam, clamp_radius=4)
    assert same(got["mean"][miss], lin[miss]) and np.all(got["sd"][miss] == 0.0) and not got["clipped"].any()
    assert (got["sd"][~miss] > 0.0).all()
    wild = lin.copy()
    wild[miss] = 1e6 * rng.standard_normal((int(miss.sum()), 3))
    other = run(wild, f, cam, clamp_radius=4)
    assert same(other["mean"][~miss], got["mean"][~miss]) and same(other["sd"][~miss], got["sd"][~miss])
    history = dict(other, cam=prev_cam)
    second = run(wild, f, cam, history=history, clamp_radius=4, gamma=0.25)
    assert same(second["mean"][miss], wild[miss]) and np.all(second["sd"][miss] == 0.0) and np.all(second["clipped"][miss] == 0)
    assert same(second["linear"][miss], wild[miss]) and same(second["moment2"][miss], (wild * wild)[miss]) and np.all(second["length"][miss] == 1.0)
    assert same(second["linear"][~miss], run(lin, f, cam, history=dict(got, cam=prev_cam), clamp_radius=4, gamma=0.25)["linear"][~miss])


def check_properties(run, unclamped):
    check_a_ghost_goes(run, unclamped)
    noise = check_noise_stays(run)
    check_the_window_respects_edges(run)
    check_miss_pixels(run)
    return noise
