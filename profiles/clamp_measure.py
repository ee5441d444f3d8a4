"""rttnw_temporal_clamp against rttnw_temporal_variance, 800x800, 4 samples a frame, an orbit of 1 degree a frame on cornell_box and final_scene.
Cost: kernel_ms of the two entry points on the same inputs — the first call of a sequence (no history: nothing to clip; with the statistics asked
for every block with a hit stages its tile, without them none does), the second call one degree on, and the sixth call of a running sequence —
at radius 1 / 3 / 4 (the clip's window and stage B's alike), and image_ms of a running rttnw_svgf handle (feedback 1, demodulate) with and without
a clamp: medians of 7 alternating runs behind a warm-up.  Events around launches of some 50 microseconds spread by 10 - 20 %.  Quality: MSE of the
last frame of the 16-frame orbit against the oracle's converged t2_* windows, demodulate on, feedback 0 / 1, clamp off / gamma 1 / gamma 3, and
the share of the hit pixels' channels each clamped sequence clipped in its last frame."""
import copy, os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from golden_cases import WINDOWS, load_windows
from rttnw_amd import abi, library, render
from rttnw_amd import scene as S

gpu = library.product()
lib = library.scenes()
REPS, FRAMES = 7, 16
W = H = 800
gold = load_windows()
for name in ("cornell_box", "final_scene"):
    sc, setup = S.build(gpu, lib, name, S.load_earth() if name == "final_scene" else None)
    cam, p = S.params_for(setup, W, H, 4, precision=abi.F64)
    cams = render.orbit_cameras(cam, FRAMES, 1.0)
    frames = []
    for k, c in enumerate(cams[-6:]):
        pk = copy.copy(p); pk.sample_begin = k * p.spp
        frames.append((render.render_host(sc, c, pk)[0], render.render_features(sc, c, pk), c))
    history = clamped = None
    for lin, f, c in frames[:5]:
        history = render.temporal_variance(lin, f, c, history=history)
        clamped = render.temporal_clamp(lin, f, c, history=clamped)
    first = render.temporal_variance(*frames[4])                       # frame 4 as the start of a sequence: the history of "one degree on"
    lin, f, c = frames[5]
    runs = {}
    for r in (1, 3, 4):
        kv, kc = dict(radius=r, want_ms=True), dict(radius=r, clamp_radius=r, want_ms=True)
        runs.update({
            "temporal_variance, no history, radius %d" % r: lambda kv=kv: render.temporal_variance(lin, f, c, **kv)["ms"],
            "temporal_clamp,    no history, radius %d" % r: lambda kc=kc: render.temporal_clamp(lin, f, c, **kc)["ms"],
            "temporal_clamp,    no history, radius %d, no statistics" % r: lambda kc=kc: render.temporal_clamp(lin, f, c, want_statistics=False, **kc)["ms"],
            "temporal_variance, 1 degree on, 2nd frame, radius %d" % r: lambda kv=kv: render.temporal_variance(lin, f, c, history=first, **kv)["ms"],
            "temporal_clamp,    1 degree on, 2nd frame, radius %d" % r: lambda kc=kc: render.temporal_clamp(lin, f, c, history=first, want_statistics=False, **kc)["ms"],
            "temporal_variance, 1 degree on, running, radius %d" % r: lambda kv=kv: render.temporal_variance(lin, f, c, history=history, **kv)["ms"],
            "temporal_clamp,    1 degree on, running, radius %d" % r: lambda kc=kc: render.temporal_clamp(lin, f, c, history=clamped, want_statistics=False, **kc)["ms"]})
    ms = {k: [] for k in runs}
    for k in runs: runs[k]()                      # warm-up of every shape
    for _ in range(REPS):                         # alternating
        for k in runs: ms[k].append(runs[k]())
    for k in runs:
        print("%s f64 800x800 %-62s kernel_ms median %.3f (min %.3f max %.3f)" % (name, k, statistics.median(ms[k]), min(ms[k]), max(ms[k])), flush=True)
    last = render.temporal_clamp(lin, f, c, history=clamped)
    hit = f["alpha"] != 0.0
    print("%s: running sequence at the defaults (gamma 1, radius 3): %.1f %% of the pixels hit, %.2f %% of their channels were clipped"
          % (name, 100.0 * hit.mean(), 100.0 * np.unpackbits(last["clipped"][hit][:, None], axis=1).sum() / (3.0 * hit.sum())), flush=True)
    # where the interval is narrow: a window whose neighbours weigh nothing (a silhouette, a curved surface under sigma_normal 64) has sd near 0
    moved = np.stack([(last["clipped"] >> ch) & 1 for ch in range(3)], axis=-1).astype(bool)
    narrow = last["sd"] <= 1e-3 * np.abs(last["mean"])
    blended = hit & (last["length"] > 1.0)
    print("%s: same call: %.2f %% of the blended pixels' channels have sd <= mean / 1000; they are %.1f %% of the clipped channels; gamma 3 on the same history "
          "clips %.2f %% of the hit pixels' channels" % (name, 100.0 * narrow[blended].mean(), 100.0 * (moved & narrow).sum() / max(moved.sum(), 1),
                                                      100.0 * np.unpackbits(render.temporal_clamp(lin, f, c, history=clamped, gamma=3.0)["clipped"][hit][:, None], axis=1).sum()
                                                      / (3.0 * hit.sum())), flush=True)

    handle = {"handle, feedback 1, albedo, no clamp": None, "handle, feedback 1, albedo, clamp gamma 1": 1.0}
    image_ms = {k: [] for k in handle}
    sequence = lambda g: render.render_sequence_device(sc, cams[-6:], p, feedback=1, demodulate=True, want=("rgba8",), clamp=g)
    for k, g in handle.items(): sequence(g)       # warm-up
    for _ in range(REPS):
        for k, g in handle.items():
            image_ms[k].append(statistics.median(fr["image_ms"] for fr in sequence(g)[1:]))
    for k in handle:
        print("%s f64 800x800 %-62s image_ms a frame median %.3f (min %.3f max %.3f)" % (name, k, statistics.median(image_ms[k]), min(image_ms[k]), max(image_ms[k])),
              flush=True)

    images, shares = {}, {}
    for feedback in (0, 1):
        for g in (None, 1.0, 3.0):
            key = "feedback %d, %s" % (feedback, "no clamp" if g is None else "gamma %g" % g)
            got = render.render_sequence_device(sc, cams, p, feedback=feedback, demodulate=True, want=("linear_rgb", "alpha"), clamp=g)[-1]
            images[key] = got["linear"]
            if g is not None:
                bits, on = got["clipped"], got["features"]["alpha"] != 0.0
                shares[key] = (100.0 * np.unpackbits((bits & 7)[on][:, None], axis=1).sum() / (3.0 * on.sum()),
                               100.0 * np.unpackbits((bits >> 4)[on][:, None], axis=1).sum() / (3.0 * on.sum()))
    for key, (m1, hh) in shares.items():
        print("%s last frame, %s: %.2f %% of the hit pixels' channels clipped in M1, %.2f %% in H" % (name, key, m1, hh), flush=True)
    for key, scene, w, h, spp, x0, y0, cw, ch, _ in WINDOWS:
        if scene != name or not key.startswith("t2_"):
            continue
        ref = gold[key + "_linear"]
        crop = (slice(y0, y0 + ch), slice(x0, x0 + cw))
        print("%s MSE: %s" % (key, "; ".join("%s %.4g" % (k, float(np.mean((v[crop] - ref) ** 2))) for k, v in images.items())), flush=True)
