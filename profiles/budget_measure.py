"""Three renders of equal traced samples, 800x800, f64, against the committed oracle windows: uniform rttnw_render, rttnw_render_adaptive under the
tolerance that happens to trace that many, and rttnw_render_adaptive_budget — for rounds of an eighth, a quarter and a half of the frame; and the
selection's device time per round (rttnw_budget_select on the final maps) next to the round's share of the call's kernel_ms."""
import copy, os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from golden_cases import WINDOWS, load_windows
from rttnw_amd import abi, library, render
from rttnw_amd import scene as S

gpu = library.product()
lib = library.scenes()
W = H = 800
B, CAP, MEAN_SPP, REL, ABS = 16, 512, 64, 0.02, 0.002
BUDGET = W * H * MEAN_SPP
REPS = 5
gold = load_windows()


def errors(name, img):
    """Mean and 99th percentile, over the pixels of the scene's oracle windows, of |luminance - oracle's| / (oracle's + 0.01)."""
    rel = []
    for key, scene, w, h, _, x0, y0, cw, ch, _ in WINDOWS:
        if scene != name or not key.startswith("t2_"): continue
        ref = gold[key + "_linear"].mean(axis=2); got = img[y0:y0 + ch, x0:x0 + cw].mean(axis=2)
        rel.append((np.abs(got - ref) / (ref + 0.01)).reshape(-1))
    rel = np.concatenate(rel)
    return float(rel.mean()), float(np.percentile(rel, 99))


for name in ("cornell_box", "final_scene"):
    sc, setup = S.build(gpu, lib, name, S.load_earth() if name == "final_scene" else None)
    cam, p = S.params_for(setup, W, H, CAP, precision=abi.F64)
    pu = copy.copy(p); pu.spp = MEAN_SPP
    render.render_host(sc, cam, pu)                                      # warm-up
    lin, _, st = render.render_host(sc, cam, pu)
    print("%s uniform %d spp: %d samples, kernel_ms %.1f, rel error mean %.4f p99 %.4f" % ((name, MEAN_SPP, st.samples, st.kernel_ms) + errors(name, lin)), flush=True)
    # the tolerance under which the adaptive render traces the budget: bisection on rel_error (samples fall as it grows)
    lo, hi = 0.005, 2.0
    for _ in range(14):
        mid = (lo * hi) ** 0.5
        n = render.render_adaptive(sc, cam, p, pass_spp=B, rel_error=mid, abs_error=ABS)[4].samples
        lo, hi = (mid, hi) if n > BUDGET else (lo, mid)
    lin, _, spp, _, st = render.render_adaptive(sc, cam, p, pass_spp=B, rel_error=hi, abs_error=ABS)
    print("%s adaptive rel_error %.4f: %d samples (%.3f of the budget), kernel_ms %.1f, rel error mean %.4f p99 %.4f; %.3f of the pixels at the cap"
          % ((name, hi, st.samples, st.samples / BUDGET, st.kernel_ms) + errors(name, lin) + (float((spp == CAP).mean()),)), flush=True)
    runs = {frac: (lambda rp=W * H // frac: render.render_adaptive_budget(sc, cam, p, BUDGET, rp, pass_spp=B, rel_error=REL, abs_error=ABS, want_state=False))
            for frac in (8, 4, 2)}
    ms = {k: [] for k in runs}
    for k in runs: runs[k]()
    for _ in range(REPS):                                                # alternating
        for k in runs:
            out = runs[k](); ms[k].append(out[4].kernel_ms)
    for frac in runs:
        lin, _, spp, se, st, _, rounds = runs[frac]()
        sel = []
        for _ in range(REPS):
            sel.append(render.budget_select(lin, se, spp, CAP, REL, ABS, W * H // frac, want_ms=True)[3])
        m = statistics.median(ms[frac])
        print("%s budget rounds of 1/%d frame: %d samples in %d rounds, kernel_ms median %.1f (min %.1f max %.1f), rel error mean %.4f p99 %.4f; "
              "selection %.3f ms per round (median of %d, min %.3f max %.3f) beside %.2f ms of the call per round; spp max %d, %.3f of the pixels at the cap"
              % ((name, frac, st.samples, rounds, m, min(ms[frac]), max(ms[frac])) + errors(name, lin) +
                 (statistics.median(sel), REPS, min(sel), max(sel), m / rounds, int(spp.max()), float((spp == CAP).mean()))), flush=True)
