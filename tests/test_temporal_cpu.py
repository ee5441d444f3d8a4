"""rttnw_temporal_accumulate without a GPU: the host build of the arithmetic the device kernel runs (rttnw_amd/csrc/temporal.hpp, built by
tests/temporal_host) against a numpy restatement of the contract in include/rttnw_hip.h — bit for bit, every output — and the properties the
contract promises: no history and equal cameras, the running mean of a static camera, the reprojection against an independent formula, exact
bilinear interpolation, and disocclusions rejected by depth and by normal."""
import numpy as np
import pytest

import denoise_ref
import temporal_ref
from temporal_cases import (CASE_IDS, CASES, H, W, analytic_pair, assert_same_outputs, cameras, case_parameters, check_disocclusion,
                            check_no_history_and_equal_cameras, check_running_mean, classify, project, random_case, running_mean_frames)


@pytest.fixture(scope="module")
def host():
    return temporal_ref.host()


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_host_build_equals_the_numpy_restatement_bit_for_bit(host, case):
    lin, f, cam, history, var = random_case(case)
    kw = case_parameters(case)
    got = host(lin, f, cam, history=history, variance=var, **kw)
    assert_same_outputs(got, temporal_ref.accumulate(lin, f, cam, history=history, variance=var, **kw))
    if case[0] == (70, 41) and case[4] and case[2] > 1:   # the accepting branch was exercised: blends, and resets beside them
        hit = f["alpha"] != 0.0
        assert (got["length"][hit] > 1.0).mean() > 0.25
        assert (got["length"] == 1.0)[np.isfinite(got["prev_xy"][..., 0])].any()
    # ... and a second step over the first one's result, at the other tolerance
    nxt = host(history["linear"], history["features"], history["cam"], history=got, variance=history["variance"], depth_tolerance=0.2, **kw)
    assert_same_outputs(nxt, temporal_ref.accumulate(history["linear"], history["features"], history["cam"], history=got, variance=history["variance"],
                                                     depth_tolerance=0.2, **kw))


def test_zero_parameters_are_the_stated_defaults(host):
    lin, f, cam, history, var = random_case(((70, 41), True, 32, 0.0, True))
    default = host(lin, f, cam, history=history, variance=var)
    assert_same_outputs(default, host(lin, f, cam, history=history, variance=var, max_history=32, depth_tolerance=0.05, normal_min=0.9))
    assert not np.array_equal(default["length"], host(lin, f, cam, history=history, variance=var, normal_min=-1.0)["length"])


def test_no_history_and_equal_cameras(host):
    check_no_history_and_equal_cameras(host)
    check_no_history_and_equal_cameras(temporal_ref.accumulate)


def test_a_static_camera_accumulates_the_running_mean(host):
    rng = np.random.default_rng(3)
    w, h = 37, 29
    f = denoise_ref.random_inputs(rng, w, h, False)[2]
    check_running_mean(host, running_mean_frames(rng, w, h, 8), f, cameras(w / h)[0])


def test_the_reprojection_agrees_with_an_independent_formula(host):
    """out_prev_xy — the record's lower_left_corner, horizontal and vertical — against the projection through the orthonormal basis and
    tan(fov / 2), on the analytic scene: within 1e-9 pixels (the two forms differ by 3e-14 in numpy)."""
    cur, prev, f, pf, points = analytic_pair()
    classes, fx, fy, _, _ = classify(points, prev, pf)
    lin = np.zeros((H, W, 3))
    history = {"linear": lin, "variance": None, "length": np.ones((H, W)), "features": pf, "cam": prev}
    got = host(lin, f, cur, history=history)
    inside = (fx > -1.0 + 1e-6) & (fx < W - 1e-6) & (fy > -1.0 + 1e-6) & (fy < H - 1e-6)
    assert inside.sum() > 1300 and np.isfinite(got["prev_xy"][inside]).all()
    assert np.abs(got["prev_xy"][inside] - np.stack([fx, fy], axis=-1)[inside]).max() < 1e-9
    beyond = (fx < -1.0 - 1e-6) | (fx > W + 1e-6) | (fy < -1.0 - 1e-6) | (fy > H + 1e-6)
    assert beyond.any() and np.isnan(got["prev_xy"][beyond]).all()
    # ... and the distance the depth test compares with
    _, _, zq = project(prev, points, W, H)
    assert np.abs(temporal_ref.where_it_was(W, H, cur, prev, f["depth"], f["alpha"])[2] - zq).max() < 1e-9


def test_bilinear_taps_reproduce_a_linear_function(host):
    """prev_linear_rgb linear in the previous pixel coordinates, prev_length 1, this frame 0: N = 2 and a = 1 / 2, so 2 * out is the function at
    (fx, fy) wherever all four taps are accepted."""
    cur, prev, f, pf, points = analytic_pair()
    classes, fx, fy, _, _ = classify(points, prev, pf)
    ys, xs = np.mgrid[0:H, 0:W]
    coefficients = np.array([[0.3, 0.01, 0.002], [1.0, -0.004, 0.03], [0.1, 0.02, 0.02]])
    plane = lambda x, y: np.stack([c0 + c1 * x + c2 * y for c0, c1, c2 in coefficients], axis=-1)
    history = {"linear": plane(xs, ys), "variance": None, "length": np.ones((H, W)), "features": pf, "cam": prev}
    got = host(np.zeros((H, W, 3)), f, cur, history=history)
    acc = classes["accepted"]
    assert acc.sum() >= 1000 and np.all(got["length"][acc] == 2.0)
    assert np.abs(2.0 * got["linear"][acc] - plane(fx, fy)[acc]).max() < 1e-9


def test_disocclusions_reset_by_depth_and_by_normal(host):
    check_disocclusion(host, temporal_ref.accumulate)
