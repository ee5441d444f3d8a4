"""kernel_ms of rttnw_denoise_nlm at 800x800 (default parameters, and r 10, f 3) beside the parent's yardsticks in the same run — the two rttnw_render
calls that make the 8-sample halves, and rttnw_denoise with five passes — on cornell_box and final_scene: medians of 7 alternating runs behind a
warm-up.  Then the quality figures in the seven oracle windows (MSE against tests/golden/golden_windows.npz)."""
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
    mean = (a + b) * 0.5
    features = render.render_features(sc, cam, p)
    runs = {"two halves of 8 spp": lambda: sum(h[2].kernel_ms for h in render.render_halves(sc, cam, p)),
            "rttnw_denoise 5 passes": lambda: render.denoise(mean, features, None, want_ms=True)[3],
            "nlm r7 f3": lambda: render.denoise_nlm(a, b, want_ms=True)["ms"],
            "nlm r10 f3": lambda: render.denoise_nlm(a, b, search_radius=10, patch_radius=3, want_ms=True)["ms"]}
    ms = {k: [] for k in runs}
    for k in runs: runs[k]()                      # warm-up of every shape
    for _ in range(REPS):                         # alternating
        for k in runs: ms[k].append(runs[k]())
    base = statistics.median(ms["two halves of 8 spp"])
    for k in runs:
        m = statistics.median(ms[k])
        print("%s f64 800x800 %-24s kernel_ms median %.2f (min %.2f max %.2f) = %.3f of the 16 samples" % (name, k, m, min(ms[k]), max(ms[k]), m / base), flush=True)
    # quality: the pair-variance flavour, the given-variance flavour (two adaptive renders run to their cap of 8), the feature-guided filter
    halves = []
    for k in range(2):
        cam_h, ph = S.params_for(setup, 800, 800, 8, precision=abi.F64, sample_begin=8 * k)
        lin, _, _, se, _ = render.render_adaptive(sc, cam_h, ph, pass_spp=8, rel_error=0.0)
        halves.append((lin, np.square(se)))
    images = {"plain 16 spp": mean, "rttnw_denoise (no variance)": render.denoise(mean, features, None)[0],
              "nlm pair variance": render.denoise_nlm(a, b)["linear"],
              "nlm given variance": render.denoise_nlm(halves[0][0], halves[1][0], halves[0][1], halves[1][1])["linear"],
              "nlm r10 f3 pair variance": render.denoise_nlm(a, b, search_radius=10, patch_radius=3)["linear"]}
    gold = load_windows()
    for key, scene, w, h, _, x0, y0, cw, ch, _ in WINDOWS:
        if scene != name or not key.startswith("t2_"): continue
        ref = gold[key + "_linear"]; crop = (slice(y0, y0 + ch), slice(x0, x0 + cw))
        print("%s: %s" % (key, ", ".join("%s %.4g" % (k, float(np.mean((img[crop] - ref) ** 2))) for k, img in images.items())), flush=True)
