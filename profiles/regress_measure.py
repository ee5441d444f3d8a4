"""rttnw_denoise_regress at 800x800, halves of 8 samples, on cornell_box and final_scene.
1. kernel_ms of rttnw_denoise_regress (masks 0 and 7, demodulation off and on) beside rttnw_denoise_nlm and rttnw_denoise in the same process:
   medians and ranges of 7 alternating runs behind a warm-up.  Mask 0 without demodulation is non-local means in the new kernel's structure.
2. The ridge sweep the library default was taken from: 1e-4, 1e-3, 1e-2, 1e-1 with features 7 and demodulation, the MSE in each of the seven
   committed oracle windows (tests/golden/golden_windows.npz) and the geometric mean over the seven.
3. The quality table: plain, rttnw_denoise, rttnw_denoise_nlm, regress without and with demodulation (default ridge), share of fit < 2."""
import os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from golden_cases import WINDOWS, load_windows
from rttnw_amd import abi, library, render
from rttnw_amd import scene as S

gpu = library.product()
lib = library.scenes()
gold = load_windows()
REPS = 7
RIDGES = (1e-4, 1e-3, 1e-2, 1e-1)
sweep = {ridge: [] for ridge in RIDGES}


def window_mse(name, img):
    out = []
    for key, scene, w, h, _, x0, y0, cw, ch, _ in WINDOWS:
        if scene == name and key.startswith("t2_"):
            out.append((key, float(np.mean((img[y0:y0 + ch, x0:x0 + cw] - gold[key + "_linear"]) ** 2))))
    return out


for name in ("cornell_box", "final_scene"):
    sc, setup = S.build(gpu, lib, name, S.load_earth() if name == "final_scene" else None)
    cam, p = S.params_for(setup, 800, 800, 16, precision=abi.F64)
    (a, _, _), (b, _, _) = render.render_halves(sc, cam, p)
    mean = (a + b) * 0.5
    f = render.render_features(sc, cam, p)
    regress = lambda **kw: render.denoise_regress(a, b, None, None, f, want_ms=True, **kw)
    runs = {"rttnw_denoise 5 passes": lambda: render.denoise(mean, f, None, want_ms=True)[3],
            "rttnw_denoise_nlm": lambda: render.denoise_nlm(a, b, want_ms=True)["ms"],
            "regress mask 0, no demodulation": lambda: regress(mask=0, demodulate=False)["ms"],
            "regress mask 0, demodulation": lambda: regress(mask=0)["ms"],
            "regress mask 7, no demodulation": lambda: regress(demodulate=False)["ms"],
            "regress mask 7, demodulation": lambda: regress()["ms"]}
    ms = {k: [] for k in runs}
    for k in runs: runs[k]()                      # warm-up of every shape
    for _ in range(REPS):                         # alternating
        for k in runs: ms[k].append(runs[k]())
    base = statistics.median(ms["rttnw_denoise_nlm"])
    for k in runs:
        m = statistics.median(ms[k])
        print("%s f64 800x800 %-34s kernel_ms median %.2f (min %.2f max %.2f) = %.2f of rttnw_denoise_nlm" % (name, k, m, min(ms[k]), max(ms[k]), m / base), flush=True)
    for ridge in RIDGES:
        rows = window_mse(name, regress(ridge=ridge)["linear"])
        sweep[ridge] += [v for _, v in rows]
        print("%s ridge %g: %s" % (name, ridge, ", ".join("%s %.4g" % kv for kv in rows)), flush=True)
    plain, demod = regress(demodulate=False), regress()
    images = {"plain 16 spp": mean, "rttnw_denoise": render.denoise(mean, f, None)[0], "rttnw_denoise_nlm": render.denoise_nlm(a, b)["linear"],
              "regress no demodulation": plain["linear"], "regress demodulation": demod["linear"]}
    table = {k: dict(window_mse(name, img)) for k, img in images.items()}
    for key, scene, w, h, _, x0, y0, cw, ch, _ in WINDOWS:
        if scene != name or not key.startswith("t2_"): continue
        print("%s: %s, fit < 2 on %.2f %% of the window" % (key, ", ".join("%s %.4g" % (k, table[k][key]) for k in images),
                                                          100.0 * float((demod["fit"][y0:y0 + ch, x0:x0 + cw] < 2.0).mean())), flush=True)
    print("%s: fit < 2 on %.2f %% of the frame, fit == 0 on %.2f %%" % (name, 100.0 * float((demod["fit"] < 2.0).mean()), 100.0 * float((demod["fit"] == 0.0).mean())), flush=True)
for ridge in RIDGES:
    print("ridge %g: geometric mean of the seven window MSEs %.5g" % (ridge, float(np.exp(np.mean(np.log(sweep[ridge]))))), flush=True)
