"""kernel_ms of rttnw_denoise_select at 800x800 (everything at its default, and the largest selection radii) beside the calls it is made of in the
same run — rttnw_denoise with five passes, rttnw_denoise_nlm — and the two rttnw_render calls that make the 8-sample halves, on cornell_box and
final_scene: medians of 7 alternating runs behind a warm-up.  The selection's own kernels are what the call costs beyond two rttnw_denoise runs
and one rttnw_denoise_nlm run (whose finish kernel the call does not run: the difference is a lower bound by that kernel's time; a kernel trace
of this script gives the two selection kernels directly).  Then the quality figures in the seven oracle windows (MSE against
tests/golden/golden_windows.npz) and the share of each window that went to non-local means."""
import os, sys, statistics
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
    cam, p = S.params_for(setup, 800, 800, 16, precision=abi.F64)
    (a, _, _), (b, _, _) = render.render_halves(sc, cam, p)
    features = render.render_features(sc, cam, p)
    runs = {"two halves of 8 spp": lambda: sum(h[2].kernel_ms for h in render.render_halves(sc, cam, p)),
            "rttnw_denoise 5 passes": lambda: render.denoise(a, features, None, want_ms=True)[3],
            "nlm r7 f3": lambda: render.denoise_nlm(a, b, want_ms=True)["ms"],
            "select s5 t2": lambda: render.denoise_select(a, b, features, want_ms=True)["ms"],
            "select s16 t8": lambda: render.denoise_select(a, b, features, error_radius=16, blend_radius=8, want_ms=True)["ms"]}
    ms = {k: [] for k in runs}
    for k in runs: runs[k]()                      # warm-up of every shape
    for _ in range(REPS):                         # alternating
        for k in runs: ms[k].append(runs[k]())
    med = {k: statistics.median(ms[k]) for k in runs}
    for k in runs:
        print("%s f64 800x800 %-24s kernel_ms median %.2f (min %.2f max %.2f) = %.3f of the 16 samples"
              % (name, k, med[k], min(ms[k]), max(ms[k]), med[k] / med["two halves of 8 spp"]), flush=True)
    parts = 2.0 * med["rttnw_denoise 5 passes"] + med["nlm r7 f3"]
    for k in ("select s5 t2", "select s16 t8"):
        print("%s f64 800x800 %-24s beyond two rttnw_denoise and one rttnw_denoise_nlm (%.2f ms): %.2f ms" % (name, k, parts, med[k] - parts), flush=True)
    out = render.denoise_select(a, b, features)
    level = render.denoise_select(a, b, features, margin=0.0)
    gold = load_windows()
    for key, scene, w, h, _, x0, y0, cw, ch, _ in WINDOWS:
        if scene != name or not key.startswith("t2_"): continue
        ref = gold[key + "_linear"]; crop = (slice(y0, y0 + ch), slice(x0, x0 + cw))
        mse = lambda img: float(np.mean((img[crop] - ref) ** 2))
        print("%s: feature-guided %.4g, non-local means %.4g, selected %.4g (mean beta %.3f), selected at margin 0 %.4g (mean beta %.3f)"
              % (key, mse(out["feature"]), mse(out["nlm"]), mse(out["linear"]), out["blend"][crop].mean(), mse(level["linear"]), level["blend"][crop].mean()),
              flush=True)
    print("%s: %.1f %% of the frame took non-local means, %.1f %% the feature-guided filter" % (name, 100.0 * (out["blend"] == 1.0).mean(),
                                                                                           100.0 * (out["blend"] == 0.0).mean()), flush=True)
