"""What the tests of rttnw_temporal_accumulate share (tests/test_temporal_cpu.py on the host harness, tests/test_gpu_temporal.py on the device): the
frames, cameras and parameter sets both are held to, the analytic two-plane scene with its independent projection, and the checks of the
properties both must have.  An implementation under test is a function
run(linear, features, cam, history=None, variance=None, **parameters) -> dict of temporal_ref.OUTPUTS plus "features" and "cam", so that a result
is the next call's history."""
import numpy as np

import denoise_ref
import temporal_ref
from rttnw_amd import scene as S

SIZES = [(1, 1), (3, 5), (37, 29), (70, 41)]     # 70 crosses the device's 64-wide blocks, 1x1 and 3x5 are smaller than one
# (size, with variances, max_history, normal_min, depths from the analytic scene): every size with every setting, half of them analytic
CASES = [(size, v, mh, nm, (i + j + k + m) % 2 == 0) for i, size in enumerate(SIZES) for j, v in enumerate((True, False))
         for k, mh in enumerate((1, 4, 32)) for m, nm in enumerate((-1.0, 0.0))]
CASE_IDS = ["%dx%d-%s-h%d-%s-%s" % (s[0], s[1], "variance" if v else "plain", mh, "no-normal-test" if nm == -1.0 else "normal-test",
                                     "analytic" if an else "random") for s, v, mh, nm, an in CASES]
W, H = 48, 32                                     # the analytic scene's frame
STRIP_Z, STRIP_HALF_WIDTH = 3.0, 0.7


def cameras(aspect):
    """(this frame's camera, the previous frame's): a few degrees and a fraction of the scene apart."""
    cur = S.camera_desc(lookfrom=(0.0, 0.2, 9.0), lookat=(0.0, 0.0, 0.0), vfov=40.0, aspect=aspect, view_up=(0.0, 1.0, 0.0), focus=10.0)
    prev = S.camera_desc(lookfrom=(0.6, 0.1, 8.7), lookat=(0.1, 0.0, 0.0), vfov=40.0, aspect=aspect, view_up=(0.02, 1.0, 0.0), focus=7.0)
    return cur, prev


def same(a, b):
    """The same bits, a NaN standing for any NaN (an arithmetic NaN's sign and payload are the processor's)."""
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float64:
        return np.array_equal(a, b)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(np.where(na, 0.0, a).view(np.uint64), np.where(nb, 0.0, b).view(np.uint64))


def assert_same_outputs(got, want, what=()):
    for name in temporal_ref.OUTPUTS:
        assert same(got[name], want[name]), (name,) + tuple(what)


# ---- the projection written through the orthonormal basis and tan(fov / 2): independent of the record's lower_left_corner, horizontal, vertical

def _basis(cam):
    o, at, up = (np.array(v[:], dtype=np.float64) for v in (cam.lookfrom, cam.lookat, cam.view_up))
    unit = lambda v: v / np.sqrt(np.dot(v, v))
    w = unit(o - at)
    u = unit(np.cross(up, w))
    v = np.cross(w, u)
    half_h = np.tan(np.deg2rad(cam.vertical_fov) / 2.0)
    return o, u, v, w, cam.aspect_ratio * half_h, half_h


def pixel_rays(cam, w, h):
    """(origin, directions HxWx3, not normalised) of the pixel-centre rays."""
    o, u, v, back, half_w, half_h = _basis(cam)
    ys, xs = np.mgrid[0:h, 0:w]
    s, t = (xs + 0.5) / w, ((h - 1 - ys) + 0.5) / h
    return o, ((2.0 * s - 1.0) * half_w)[..., None] * u + ((2.0 * t - 1.0) * half_h)[..., None] * v - back


def project(cam, points, w, h):
    """(fx, fy) of world points in `cam`'s pixel coordinates, and their distance from its origin."""
    o, u, v, back, half_w, half_h = _basis(cam)
    rel = points - o
    forward = -(rel @ back)
    fx = ((rel @ u) / (forward * half_w) + 1.0) * 0.5 * w - 0.5
    fy = h - ((rel @ v) / (forward * half_h) + 1.0) * 0.5 * h - 0.5
    return fx, fy, np.sqrt(np.sum(rel * rel, axis=-1))


def analytic_scene(cam, w, h, strip_normal=(0.0, 0.0, 1.0)):
    """A back plane z = 0 and a front strip z = 3 for |x| < 0.7, seen through the pixel-centre rays of `cam`: (features, hit points HxWx3, on the strip HxW)."""
    o, d = pixel_rays(cam, w, h)
    t_front = (STRIP_Z - o[2]) / d[..., 2]
    on_strip = np.abs(o[0] + t_front * d[..., 0]) < STRIP_HALF_WIDTH
    t = np.where(on_strip, t_front, (0.0 - o[2]) / d[..., 2])
    points = o + t[..., None] * d
    normal = np.where(on_strip[..., None], np.array(strip_normal, dtype=np.float64), np.array([0.0, 0.0, 1.0]))
    depth = t * np.sqrt(np.sum(d * d, axis=-1))
    return {"albedo": np.ones((h, w, 3)), "normal": normal, "depth": depth, "alpha": np.ones((h, w))}, points, on_strip


def analytic_pair(strip_normal=(0.0, 0.0, 1.0), w=W, h=H):
    cur, prev = cameras(w / h)
    f, points, _ = analytic_scene(cur, w, h, strip_normal)
    pf, _, _ = analytic_scene(prev, w, h, strip_normal)
    return cur, prev, f, pf, points


def classify(points, prev_cam, prev_features, w=W, h=H, depth_tolerance=0.05):
    """From the analytic depths alone: per pixel "accepted" (all four taps inside the image and at the reprojected distance), "rejected" (all four
    inside, none at it), otherwise "mixed" or "outside" (the reprojection, or one of its taps, leaves the image); and (fx, fy)."""
    fx, fy, zq = project(prev_cam, points, w, h)
    x0, y0 = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
    inside = (x0 >= 0) & (x0 + 1 < w) & (y0 >= 0) & (y0 + 1 < h)
    agree = np.zeros((4, h, w), dtype=bool)
    error = np.full((4, h, w), np.nan)
    for k, (i, j) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        z = prev_features["depth"][np.clip(y0 + j, 0, h - 1), np.clip(x0 + i, 0, w - 1)]
        error[k] = np.abs(z - zq) / zq
        agree[k] = error[k] <= depth_tolerance
    classes = {"accepted": inside & agree.all(axis=0), "rejected": inside & ~agree.any(axis=0), "outside": ~inside}
    classes["mixed"] = inside & ~classes["accepted"] & ~classes["rejected"]
    return classes, fx, fy, error, agree & inside


# ---- random frames

def random_case(case):
    """(linear, features, cam, history, variance) of a case of CASES: colours and variances finite; features with alpha 0, fractional alpha and short
    normals; history lengths that are 0 in places; depths random (most taps fail) or the analytic scene's (most are accepted)."""
    (w, h), with_variance, max_history, normal_min, analytic = case
    rng = np.random.default_rng(w * 1000 + h * 10 + int(with_variance) * 5 + max_history + int(normal_min))
    cur_cam, prev_cam = cameras(w / h)
    f = denoise_ref.random_inputs(rng, w, h, False)[2]
    pf = denoise_ref.random_inputs(rng, w, h, False)[2]
    if analytic:
        for feats, cam in ((f, cur_cam), (pf, prev_cam)):
            feats["depth"] = analytic_scene(cam, w, h)[0]["depth"] * feats["alpha"]      # stored depth: summed over the hits, divided by all samples
        pf["normal"] = f["normal"] + 0.02 * rng.standard_normal((h, w, 3))
    lin, prev_lin = rng.exponential(1.0, size=(h, w, 3)), rng.exponential(1.0, size=(h, w, 3))
    var = rng.exponential(0.1, size=(h, w, 3)) if with_variance else None
    history = {"linear": prev_lin, "variance": rng.exponential(0.1, size=(h, w, 3)) if with_variance else None,
               "length": rng.choice([0.0, 1.0, 1.0, 2.5, 7.0, 31.0, 40.0], size=(h, w)), "features": pf, "cam": prev_cam}
    return lin, f, cur_cam, history, var


def case_parameters(case):
    return dict(max_history=case[2], normal_min=case[3])


# ---- properties

def check_no_history_and_equal_cameras(run):
    rng = np.random.default_rng(7)
    w, h = 37, 29
    cam, _ = cameras(w / h)
    f = denoise_ref.random_inputs(rng, w, h, False)[2]
    lin, var = rng.exponential(1.0, size=(h, w, 3)), rng.exponential(0.1, size=(h, w, 3))
    for variance in (None, var):
        first = run(lin, f, cam, variance=variance)
        assert same(first["linear"], lin) and same(first["variance"], variance)
        assert np.all(first["length"] == 1.0) and np.isnan(first["prev_xy"]).all()
        assert np.array_equal(first["rgba8"], denoise_ref.quantise(lin))
        again = type(cam).from_buffer_copy(cam)                        # another object, the same 15 doubles
        second = run(rng.exponential(1.0, size=(h, w, 3)), f, again, history=first, variance=variance)
        ys, xs = np.mgrid[0:h, 0:w]
        hit = f["alpha"] != 0.0
        assert hit.any() and not hit.all()
        assert np.array_equal(second["prev_xy"][hit], np.stack([xs, ys], axis=-1)[hit].astype(np.float64))
        assert np.isnan(second["prev_xy"][~hit]).all() and np.all(second["length"][~hit] == 1.0)
        assert np.all(second["length"][hit] == 2.0)


def running_mean_frames(rng, w, h, count):
    return [rng.exponential(1.0, size=(h, w, 3)) for _ in range(count)]


def check_running_mean(run, frames, features, cam, close=1e-12):
    """A static camera and one feature set: after K frames every pixel that hit something has length K and holds the frames' mean (rounding alone:
    K steps of a two-product blend); with max_history 4 the length stops at 4 and the image is the exponential average the contract states."""
    count = len(frames)
    hit = np.asarray(features["alpha"]) != 0.0
    for most in (count, 4):
        history, want = None, None
        for k, lin in enumerate(frames):
            history = run(lin, features, cam, history=history, max_history=most)
            a = 1.0 / min(k + 1, most)
            want = lin.copy() if want is None else (1.0 - a) * want + a * lin
        assert np.all(history["length"][hit] == float(min(count, most))), most
        if most == count:
            want = np.mean(frames, axis=0)
        assert np.all(np.abs(history["linear"][hit] - want[hit]) <= close * np.abs(want[hit]) + close), most
        assert same(history["linear"][~hit], frames[-1][~hit])          # a miss passes through
        assert np.array_equal(history["prev_xy"][hit], np.argwhere(hit)[:, ::-1].astype(np.float64))


def check_disocclusion(run, reference):
    """The analytic scene at depth_tolerance 0.05: where every tap is rejected the output is this frame with length 1, where every tap is accepted
    the length is 2; everything equals `reference` (the numpy restatement).  Then the same pixels rejected by the normal test alone."""
    rng = np.random.default_rng(11)
    cur, prev, f, pf, points = analytic_pair()
    classes, _, _, error, agree = classify(points, prev, pf)
    counts = {k: int(v.sum()) for k, v in classes.items()}
    assert counts["rejected"] >= 30 and counts["accepted"] >= 1000, counts          # (40, 1267, 64 mixed and 165 outside)
    inside = ~classes["outside"]
    assert error[:, inside][agree[:, inside]].max() < 0.02 and error[:, inside][~agree[:, inside]].min() > 0.3   # no tap near the threshold
    lin = rng.exponential(1.0, size=(H, W, 3))
    history = {"linear": rng.exponential(1.0, size=(H, W, 3)), "variance": None, "length": np.ones((H, W)), "features": pf, "cam": prev}
    got = run(lin, f, cur, history=history, depth_tolerance=0.05)
    assert_same_outputs(got, reference(lin, f, cur, history=history, depth_tolerance=0.05))
    assert np.all(got["length"][classes["rejected"]] == 1.0) and same(got["linear"][classes["rejected"]], lin[classes["rejected"]])
    assert np.all(got["length"][classes["accepted"]] == 2.0)
    assert np.isfinite(got["prev_xy"][classes["rejected"]]).all()                    # a motion vector even where every tap was rejected
    # depth says nothing (tolerance 10), the strip faces +x: the normal test rejects the same pixels, and without it nothing is rejected
    cur, prev, f, pf, points = analytic_pair(strip_normal=(1.0, 0.0, 0.0))
    history = dict(history, features=pf)
    got = run(lin, f, cur, history=history, depth_tolerance=10.0)
    assert_same_outputs(got, reference(lin, f, cur, history=history, depth_tolerance=10.0))
    assert np.all(got["length"][classes["rejected"]] == 1.0) and same(got["linear"][classes["rejected"]], lin[classes["rejected"]])
    assert np.all(got["length"][classes["accepted"]] == 2.0)
    off = run(lin, f, cur, history=history, depth_tolerance=10.0, normal_min=-1.0)
    assert np.all(off["length"][inside] == 2.0)
    return counts
