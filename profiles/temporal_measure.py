"""kernel_ms of rttnw_temporal_accumulate at 800x800 — a moving camera (1 degree of the orbit between the two frames: four bilinear taps a pixel),
a static one (the geometry skipped), both with and without variances, and the first call of a sequence (no history) — beside rttnw_denoise with
five passes, the filter it sits next to, and the 4-sample render of a frame, on cornell_box and final_scene: medians of 7 alternating runs behind
a warm-up.  Then the quality figures of an 8-frame orbit of 4 samples a frame in the seven oracle windows (MSE against
tests/golden/golden_windows.npz): the last frame alone, the accumulated one, and both after rttnw_denoise."""
import copy, os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from golden_cases import WINDOWS, load_windows
from rttnw_amd import abi, library, render
from rttnw_amd import scene as S

gpu = library.product()
lib = library.scenes()
REPS = 7
for name in ("cornell_box", "final_scene"):
    sc, setup = S.build(gpu, lib, name, S.load_earth() if name == "final_scene" else None)
    cam, p = S.params_for(setup, 800, 800, 4, precision=abi.F64)
    prev_cam = render.orbit_cameras(cam, 2, 1.0)[0]
    p1 = copy.copy(p); p1.sample_begin = p.spp
    a, b = render.render_host(sc, prev_cam, p)[0], render.render_host(sc, cam, p1)[0]
    fa, fb = render.render_features(sc, prev_cam, p), render.render_features(sc, cam, p1)
    va, vb = np.full_like(a, 0.01), np.full_like(b, 0.01)
    moving = render.temporal_accumulate(a, fa, prev_cam, variance=va)
    static = render.temporal_accumulate(a, fb, cam, variance=va)
    plain = lambda h: dict(h, variance=None)
    runs = {"render of 4 spp": lambda: render.render_host(sc, cam, p1)[2].kernel_ms,
            "rttnw_denoise 5 passes": lambda: render.denoise(b, fb, None, want_ms=True)[3],
            "temporal, no history": lambda: render.temporal_accumulate(b, fb, cam, want_ms=True)["ms"],
            "temporal, moving": lambda: render.temporal_accumulate(b, fb, cam, history=plain(moving), want_ms=True)["ms"],
            "temporal, moving, variances": lambda: render.temporal_accumulate(b, fb, cam, history=moving, variance=vb, want_ms=True)["ms"],
            "temporal, static": lambda: render.temporal_accumulate(b, fb, cam, history=plain(static), want_ms=True)["ms"],
            "temporal, static, variances": lambda: render.temporal_accumulate(b, fb, cam, history=static, variance=vb, want_ms=True)["ms"]}
    ms = {k: [] for k in runs}
    for k in runs: runs[k]()                      # warm-up of every shape
    for _ in range(REPS):                         # alternating
        for k in runs: ms[k].append(runs[k]())
    for k in runs:
        print("%s f64 800x800 %-30s kernel_ms median %.3f (min %.3f max %.3f)" % (name, k, statistics.median(ms[k]), min(ms[k]), max(ms[k])), flush=True)
    out = render.temporal_accumulate(b, fb, cam, history=plain(moving))
    hit = fb["alpha"] != 0.0
    print("%s: 1 degree apart, %.1f %% of the pixels that hit found a history, %.1f %% were reset or left the frame"
          % (name, 100.0 * (out["length"][hit] == 2.0).mean(), 100.0 * (out["length"][hit] == 1.0).mean()), flush=True)
    last = render.render_sequence(sc, render.orbit_cameras(cam, 8, 1.0), p)[-1]
    images = {"single": last["raw"], "accumulated": last["linear"], "single denoised": render.denoise(last["raw"], last["features"])[0],
              "accumulated denoised": render.denoise(last["linear"], last["features"])[0]}
    gold = load_windows()
    for key, scene, w, h, _, x0, y0, cw, ch, _ in WINDOWS:
        if scene != name or not key.startswith("t2_"): continue
        ref = gold[key + "_linear"]; crop = (slice(y0, y0 + ch), slice(x0, x0 + cw))
        mse = {k: float(np.mean((v[crop] - ref) ** 2)) for k, v in images.items()}
        print("%s: single %.4g, accumulated %.4g (%.3f), denoised single %.4g, denoised accumulated %.4g (%.3f), mean history %.2f frames"
              % (key, mse["single"], mse["accumulated"], mse["accumulated"] / mse["single"], mse["single denoised"], mse["accumulated denoised"],
                 mse["accumulated denoised"] / mse["single denoised"], last["length"][crop].mean()), flush=True)
