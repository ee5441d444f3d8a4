"""What the tests of rttnw_temporal_variance share (tests/test_variance_cpu.py on the host harness, tests/test_gpu_variance.py on the device): the
chains of frames both are held to and the checks of the properties both must have.  An implementation under test is a function
run(linear, features, cam, history=None, **parameters) -> dict of variance_ref.OUTPUTS plus "features" and "cam", so that a result is the next
call's history."""
import numpy as np

import denoise_ref
import variance_ref
from rttnw_amd import scene as S
from temporal_cases import SIZES, analytic_scene, cameras, same

RADII, MIN_TEMPORAL, MAX_HISTORY = (1, 3, 4), (2, 4), (1, 4, 32)
# (size, radius, max_history, min_temporal, normal_min, depths from the analytic scene, non-finite values): every size with every radius and every
# max_history; the other settings alternate so that each meets every size, radius and max_history; a quarter of the cases carry NaN and inf
CASES = [(size, r, mh, MIN_TEMPORAL[(i + j + k) % 2], (-1.0, 0.0)[(i + k) % 2], (j + k) % 2 == 0, (3 * i + j + k) % 4 == 0)
         for i, size in enumerate(SIZES) for j, r in enumerate(RADII) for k, mh in enumerate(MAX_HISTORY)]
CASE_IDS = ["%dx%d-r%d-h%d-t%d-%s-%s%s" % (s[0], s[1], r, mh, mt, "no-normal-test" if nm == -1.0 else "normal-test", "analytic" if an else "random",
                                           "-nonfinite" if bad else "") for s, r, mh, mt, nm, an, bad in CASES]
STAGE_A = ("linear", "rgba8", "length", "prev_xy")        # what rttnw_temporal_accumulate returns as well


def assert_same_outputs(got, want, what=()):
    for name in variance_ref.OUTPUTS:
        assert same(got[name], want[name]), (name,) + tuple(what)


def case_parameters(case):
    return dict(radius=case[1], max_history=case[2], min_temporal=case[3], normal_min=case[4])


def _poison(rng, a, count=5):
    """A handful of values of `a` set to NaN and inf."""
    flat = a.reshape(-1)
    where = rng.choice(flat.size, size=min(count, flat.size), replace=False)
    flat[where] = rng.choice([np.nan, np.inf], size=where.size)


def chain(case):
    """(history, [(linear, features, cam)] * 3) of a case: a made-up history under one camera, then three frames — the camera moved, moved again,
    then a bitwise-equal camera — so that from the second call on prev_moment2_rgb and fractional lengths are a previous call's."""
    (w, h), radius, max_history, min_temporal, normal_min, analytic, bad = case
    rng = np.random.default_rng(w * 1000 + h * 10 + radius * 100 + max_history + min_temporal)
    cur, prev = cameras(w / h)
    third = S.camera_desc(lookfrom=(-0.3, 0.25, 9.1), lookat=(0.0, 0.05, 0.0), vfov=40.0, aspect=w / h, view_up=(0.0, 1.0, 0.01), focus=9.0)
    cams = [prev, cur, third, type(third).from_buffer_copy(third)]
    feats = []
    for k, cam in enumerate(cams):
        if k == 3:
            feats.append(feats[2])
            continue
        f = denoise_ref.random_inputs(rng, w, h, False)[2]
        if analytic:
            f["depth"] = analytic_scene(cam, w, h)[0]["depth"] * f["alpha"]      # stored depth: summed over the hits, divided by all samples
            if k:
                f["normal"] = feats[0]["normal"] + 0.02 * rng.standard_normal((h, w, 3))
        feats.append(f)
    m1 = rng.exponential(1.0, size=(h, w, 3))
    history = {"linear": m1, "moment2": m1 * m1 + rng.exponential(0.1, size=(h, w, 3)),
               "length": rng.choice([0.0, 1.0, 1.0, 2.5, 7.0, 31.0, 40.0], size=(h, w)), "features": feats[0], "cam": cams[0]}
    frames = [(rng.exponential(1.0, size=(h, w, 3)), feats[k], cams[k]) for k in (1, 2, 3)]
    if bad:
        _poison(rng, history["moment2"])
        for lin, _, _ in frames:
            _poison(rng, lin)
    return history, frames


def check_chain(run, reference, stage_a, case):
    """Every output of every link equals `reference`'s bit for bit — both chains run on their own results —, and stage A's four outputs equal
    `stage_a` (rttnw_temporal_accumulate, or its restatement) without variances."""
    kw = case_parameters(case)
    ta = {k: kw[k] for k in ("max_history", "normal_min")}
    got, (want, frames) = chain(case)[0], chain(case)
    spatial = temporal = 0
    for k, (lin, f, cam) in enumerate(frames):
        nxt = run(lin, f, cam, history=got, **kw)
        want = reference(lin, f, cam, history=want, **kw)
        assert_same_outputs(nxt, want, (k,))
        plain = stage_a(lin, f, cam, history=dict(got, variance=None), **ta)
        for name in STAGE_A:
            assert same(nxt[name], plain[name]), (name, k)
        hit = np.asarray(f["alpha"]) != 0.0
        trusted = nxt["length"] >= kw["min_temporal"]
        spatial += int((hit & ~trusted).sum())
        temporal += int((hit & trusted).sum())
        assert np.all(nxt["variance"][~hit] == 0.0)
        got = nxt
    return spatial, temporal


# ---- properties on made-up frames: a flat plane seen by a static camera

def flat_features(w, h, normal=(0.0, 0.0, 1.0)):
    return {"albedo": np.ones((h, w, 3)), "normal": np.broadcast_to(np.array(normal, dtype=np.float64), (h, w, 3)).copy(), "depth": np.full((h, w), 9.0),
            "alpha": np.ones((h, w))}


def check_constant_input(run):
    """Every frame the same colour: no variance, on the spatial branch (frames 1 - 3 at the default min_temporal) and on the temporal one (4, 5)."""
    w, h = 37, 29
    cam = cameras(w / h)[0]
    f = flat_features(w, h)
    lin = np.broadcast_to(np.array([0.9, 1.3, 0.4]), (h, w, 3)).copy()
    history = None
    for k in range(5):
        history = run(lin, f, cam, history=history)
        assert np.all(history["length"] == float(k + 1))
        assert np.all(history["variance"] <= 1e-14), (k, history["variance"].max())


def noisy_frames(count, w=64, h=32):
    """`count` frames of 0.5 + sigma * normal(): sigma 0.1 in the left half, 0.3 in the right; (frames, sigma per column)."""
    rng = np.random.default_rng(1)
    sigma = np.where(np.arange(w) < w // 2, 0.1, 0.3)
    return [0.5 + sigma[None, :, None] * rng.standard_normal((h, w, 3)) for _ in range(count)], sigma


def check_temporal_branch_is_unbiased(run):
    """After 8 frames the variance of the mean, times 8, averages to sigma^2 in each half within 10 %: 3072 sample variances with 7 degrees of
    freedom have a relative standard deviation of about 1 % in their mean; a divisor of N in place of N - 1 is off by 12.5 %."""
    frames, sigma = noisy_frames(8)
    h, w = frames[0].shape[:2]
    cam, f = cameras(w / h)[0], flat_features(w, h)
    history = None
    for lin in frames:
        history = run(lin, f, cam, history=history, max_history=32)
    assert np.all(history["length"] == 8.0)
    ratios = []
    for half, s in ((slice(0, w // 2), 0.1), (slice(w // 2, w), 0.3)):
        ratios.append(float((history["variance"][:, half] * 8.0).mean() / s ** 2))
        assert abs(ratios[-1] - 1.0) < 0.1, ratios
    return ratios


def check_spatial_branch_is_unbiased(run):
    """The first of those frames alone (N = 1), radius 3: away from the image border and the sigma boundary the mean of the estimate is sigma^2
    within 10 % (with equal weights its expectation is 48/49 of it)."""
    frames, sigma = noisy_frames(1)
    h, w = frames[0].shape[:2]
    got = run(frames[0], flat_features(w, h), cameras(w / h)[0], radius=3)
    assert np.all(got["length"] == 1.0)
    ratios = []
    for half, s in ((slice(3, w // 2 - 3), 0.1), (slice(w // 2 + 3, w - 3), 0.3)):
        ratios.append(float(got["variance"][3:h - 3, half].mean() / s ** 2))
        assert abs(ratios[-1] - 1.0) < 0.1, ratios
    return ratios


def check_window_respects_edges(run):
    """Two noise-free halves of different colour whose normals are perpendicular: w_n is exactly 0 across the edge, so no variance anywhere — where an
    unweighted 7x7 window sees more than 0.01 beside the edge."""
    w = h = 32
    f = flat_features(w, h)
    f["normal"][:, w // 2:] = (1.0, 0.0, 0.0)
    lin = np.full((h, w, 3), 0.2)
    lin[:, w // 2:] = 0.8
    got = run(lin, f, cameras(1.0)[0], radius=3)
    assert np.all(got["variance"] <= 1e-14), got["variance"].max()
    box = np.zeros((h, w))
    for y in range(h):
        for x in range(w):
            win = lin[max(y - 3, 0):y + 4, max(x - 3, 0):x + 4, 0]
            box[y, x] = np.mean(win * win) - np.mean(win) ** 2
    assert np.all(box[:, w // 2 - 2:w // 2 + 2] > 0.01) and np.all(box[:, :w // 2 - 3] < 1e-14)


def check_miss_pixels(run):
    """alpha == 0: variance 0 and out_moment2 = colour^2; and a miss contributes to no neighbour's window — its colour, however wild, changes no
    other pixel's variance."""
    rng = np.random.default_rng(5)
    w, h = 37, 29
    cam = cameras(w / h)[0]
    f = flat_features(w, h)
    miss = rng.random((h, w)) < 0.2
    f["alpha"][miss] = 0.0
    lin = 0.5 + 0.1 * rng.standard_normal((h, w, 3))
    got = run(lin, f, cam, radius=4)
    assert np.all(got["variance"][miss] == 0.0) and same(got["moment2"][miss], (lin * lin)[miss])
    assert (got["variance"][~miss] > 0.0).all()
    wild = lin.copy()
    wild[miss] = 1e6 * rng.standard_normal((int(miss.sum()), 3))
    other = run(wild, f, cam, radius=4)
    assert same(other["variance"], got["variance"])
    for min_temporal in (2, 4):                                          # ... and with a history, on the temporal branch and on the spatial one
        second = run(wild, f, cam, history=other, radius=4, min_temporal=min_temporal)
        assert np.all(second["length"][~miss] == 2.0) and np.all(second["length"][miss] == 1.0)
        assert np.all(second["variance"][miss] == 0.0) and same(second["moment2"][miss], (wild * wild)[miss])
        assert same(second["variance"], run(lin, f, cam, history=got, radius=4, min_temporal=min_temporal)["variance"])


def check_properties(run):
    check_constant_input(run)
    ratios = check_temporal_branch_is_unbiased(run), check_spatial_branch_is_unbiased(run)
    check_window_respects_edges(run)
    check_miss_pixels(run)
    return ratios
