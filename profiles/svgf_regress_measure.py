"""The regression stage of the rttnw_svgf handle against the plain handle, 800x800, 4 samples a frame, an orbit of 1 degree a frame on cornell_box
and final_scene, demodulate on.  Cost: image_ms — the device time behind the trace and the feature pass — of a running sequence under the plain
(à-trous), non-local-means and regress handles, and, in the same call, kernel_ms of rttnw_denoise_regress (every feature, given variances, no
demodulation: the stage's call) and of rttnw_denoise on one frame's arrays: medians of 7 alternating runs behind a warm-up of every shape, with
the spread of each.  The stage should add the filter's cost and little else: image_ms(regress) - image_ms(plain) stands beside
kernel_ms(regress) - kernel_ms(à-trous)."""
import copy, os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from rttnw_amd import abi, library, render
from rttnw_amd import scene as S

gpu = library.product()
lib = library.scenes()
REPS, FRAMES = 7, 6
W = H = 800
for name in ("cornell_box", "final_scene"):
    sc, setup = S.build(gpu, lib, name, S.load_earth() if name == "final_scene" else None)
    cam, p = S.params_for(setup, W, H, 4, precision=abi.F64)
    cams = render.orbit_cameras(cam, 16, 1.0)[-FRAMES:]
    (ha, _, _), (hb, _, _) = render.render_halves(sc, cams[-1], p)
    f = render.render_features(sc, cams[-1], p)
    var = np.full(ha.shape, 1e-3)
    handles = {"plain": {}, "nlm": dict(spatial="nlm"), "regress": dict(spatial="regress")}
    sequence = lambda kw: statistics.median(fr["image_ms"] for fr in render.render_sequence_device(sc, cams, p, demodulate=True, want=("rgba8",), **kw)[1:])
    runs = {"image_ms, handle %s" % k: (lambda kw=kw: sequence(kw)) for k, kw in handles.items()}
    runs["kernel_ms, rttnw_denoise_regress"] = lambda: render.denoise_regress(ha, hb, var, var, f, mask=7, demodulate=False, want_ms=True)["ms"]
    runs["kernel_ms, rttnw_denoise_nlm"] = lambda: render.denoise_nlm(ha, hb, var, var, want_ms=True)["ms"]
    runs["kernel_ms, rttnw_denoise"] = lambda: render.denoise((ha + hb) * 0.5, f, iterations=5, variance=var, want_ms=True)[3]
    ms = {k: [] for k in runs}
    for k in runs: runs[k]()                      # warm-up of every shape
    for _ in range(REPS):                         # alternating
        for k in runs: ms[k].append(runs[k]())
    med = {k: statistics.median(v) for k, v in ms.items()}
    for k in runs:
        print("%s f64 800x800 %-40s median %.3f (min %.3f max %.3f)" % (name, k, med[k], min(ms[k]), max(ms[k])), flush=True)
    print("%s: image_ms(regress) - image_ms(plain) = %.3f beside kernel_ms(regress) - kernel_ms(à-trous) = %.3f; image_ms(nlm) - image_ms(plain) = %.3f beside "
          "kernel_ms(nlm) - kernel_ms(à-trous) = %.3f"
          % (name, med["image_ms, handle regress"] - med["image_ms, handle plain"], med["kernel_ms, rttnw_denoise_regress"] - med["kernel_ms, rttnw_denoise"],
             med["image_ms, handle nlm"] - med["image_ms, handle plain"], med["kernel_ms, rttnw_denoise_nlm"] - med["kernel_ms, rttnw_denoise"]), flush=True)
