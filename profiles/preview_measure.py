"""kernel_ms of level-2 and level-1 previews against rttnw_render_adaptive at the same cap, 800x800, B = cap = 64, tolerance 0; and the quality
figures of levels 1 and 2 at 16 spp in the seven oracle windows."""
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
    for prec, pname in ((abi.F64, "f64"), (abi.F32, "f32")):
        cam, p = S.params_for(setup, 800, 800, 64, precision=prec)
        runs = {"adaptive": lambda: render.render_adaptive(sc, cam, p, pass_spp=64, rel_error=0.0)[4].kernel_ms,
                "preview L2": lambda: render.render_preview(sc, cam, p, 2, pass_spp=64, rel_error=0.0, want_state=False)["stats"].kernel_ms,
                "preview L1": lambda: render.render_preview(sc, cam, p, 1, pass_spp=64, rel_error=0.0, want_state=False)["stats"].kernel_ms,
                "preview L0": lambda: render.render_preview(sc, cam, p, 0, pass_spp=64, rel_error=0.0, want_state=False)["stats"].kernel_ms,
                "features 64": lambda: render.render_features(sc, cam, p)["stats"].kernel_ms}
        ms = {k: [] for k in runs}
        for k in runs: runs[k]()                      # warm-up of every shape
        for _ in range(REPS):                         # alternating
            for k in runs: ms[k].append(runs[k]())
        base = statistics.median(ms["adaptive"])
        for k in runs:
            m = statistics.median(ms[k])
            print("%s %s 800x800 B=cap=64 %-12s kernel_ms median %.2f (min %.2f max %.2f) = %.3f of adaptive" % (name, pname, k, m, min(ms[k]), max(ms[k]), m / base), flush=True)
    # quality at 16 spp, levels 1 and 2
    cam, p = S.params_for(setup, 800, 800, 16, precision=abi.F64)
    plain, _, _ = render.render_host(sc, cam, p)
    pf = copy.copy(p); pf.spp = 16
    den, _, _ = render.denoise(plain, render.render_features(sc, cam, pf), None)
    gold = load_windows()
    for level in (1, 2):
        got = render.render_preview(sc, cam, p, level, pass_spp=16, rel_error=0.0, want_state=False)
        for key, scene, w, h, _, x0, y0, cw, ch, _ in WINDOWS:
            if scene != name or not key.startswith("t2_"): continue
            ref = gold[key + "_linear"]; crop = (slice(y0, y0 + ch), slice(x0, x0 + cw))
            mse = lambda img: float(np.mean((img[crop] - ref) ** 2))
            print("%s level %d: MSE preview %.4g, plain 16 spp %.4g, denoise of the full 16-spp frame (no variance) %.4g, valid %.4f"
                  % (key, level, mse(got["linear"]), mse(plain), mse(den), got["valid"][crop].mean()), flush=True)
