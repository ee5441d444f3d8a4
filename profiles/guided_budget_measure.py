#!/usr/bin/env python3
"""The filter-guided budgeted form, measured (DESIGN.md section 10a "filter-guided budgeted form").

cornell_box and final_scene at 800x800, f64, N = 16 * w * h traced samples, B = 4, cap 256, rel_error 0.02, abs_error 0.002, 5 filter iterations,
three ways to a denoised image of equal cost in samples:
  a  rttnw_render at 16 spp, then rttnw_denoise (no variance: the uniform render has none);
  b  rttnw_render_adaptive_budget, then rttnw_denoise on its standard errors;
  c  rttnw_render_adaptive_budget_denoised.
Quality: the mean squared error and the 99th percentile of the absolute error of the linear image over the committed spp-1000 oracle windows of
that frame (tests/golden/golden_windows.npz, t2_*).  Cost: kernel_ms of (c) beside (b) + the features + one denoise — a warm-up, then the median of
REPS alternating runs — at the default round size (half the frame) and at a quarter of it; and, per round of (c), the device time of one filter
(rttnw_reconstruct on the final maps) and one selection (rttnw_budget_select on them) beside the round's share of the call.  One JSON line each.

  python profiles/guided_budget_measure.py [--scenes cornell_box,final_scene] [--size 800] [--reps 5]
"""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell_box,final_scene")
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mean-spp", type=int, default=16)
    ap.add_argument("--pass-spp", type=int, default=4)
    ap.add_argument("--cap", type=int, default=256)
    ap.add_argument("--iterations", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    from golden_cases import WINDOWS, load_windows
    from rttnw_amd import abi, library, render
    from rttnw_amd import scene as S

    gpu = library.product()
    lib = library.scenes()
    gold = load_windows()
    W = H = args.size
    B, REL, ABS, IT = args.pass_spp, 0.02, 0.002, args.iterations
    N = W * H * args.mean_spp

    def errors(name, img):
        err = []
        for key, scene, w, h, _, x0, y0, cw, ch, _ in WINDOWS:
            if scene == name and key.startswith("t2_") and w == W and h == H:
                err.append(np.abs(img[y0:y0 + ch, x0:x0 + cw] - gold[key + "_linear"]).reshape(-1))
        err = np.concatenate(err)
        return {"mse": float(np.mean(err ** 2)), "p99": float(np.percentile(err, 99))}

    for name in args.scenes.split(","):
        sc, setup = S.build(gpu, lib, name, S.load_earth() if name == "final_scene" else None)
        cam, p = S.params_for(setup, W, H, args.cap, precision=abi.F64)
        pf = copy.copy(p)
        pf.spp = B
        pf.spp_chunk = max(1, B // 16)
        pu = copy.copy(p)
        pu.spp = args.mean_spp

        def run_a():
            lin, _, st = render.render_host(sc, cam, pu)
            f = render.render_features(sc, cam, pf)
            den, _, _, ms = render.denoise(lin, f, None, iterations=IT, want_ms=True)
            return den, lin, st.samples, st.kernel_ms + f["stats"].kernel_ms + ms, 0

        def run_b(round_pixels=0):
            lin, _, spp, se, st, _, rounds = render.render_adaptive_budget(sc, cam, p, N, round_pixels, pass_spp=B, rel_error=REL, abs_error=ABS,
                                                                           want_state=False)
            f = render.render_features(sc, cam, pf)
            den, _, _, ms = render.denoise(lin, f, se, iterations=IT, want_ms=True)
            return den, lin, st.samples, st.kernel_ms + f["stats"].kernel_ms + ms, rounds

        def run_c(round_pixels=0):
            g = render.render_adaptive_budget_denoised(sc, cam, p, N, round_pixels, pass_spp=B, rel_error=REL, abs_error=ABS, iterations=IT,
                                                       want_state=False)
            return g["linear"], g["raw_linear"], g["stats"].samples, g["stats"].kernel_ms, g["rounds"], g

        runs = {"a": run_a, "b": run_b, "c": run_c, "b_quarter": lambda: run_b(W * H // 8), "c_quarter": lambda: run_c(W * H // 8)}
        ms = {k: [] for k in runs}
        last = {}
        for k in runs:                                   # warm-up
            runs[k]()
        for _ in range(args.reps):                       # alternating
            for k in runs:
                last[k] = runs[k]()
                ms[k].append(last[k][3])
        for k in runs:
            den, raw, samples, _, rounds = last[k][:5]
            print(json.dumps(dict({"what": k, "scene": name, "size": W, "samples": int(samples), "of": N, "rounds": int(rounds),
                                   "kernel_ms_median": round(statistics.median(ms[k]), 2), "kernel_ms_min": round(min(ms[k]), 2),
                                   "kernel_ms_max": round(max(ms[k]), 2), "raw": errors(name, raw)}, **errors(name, den))), flush=True)
        # per round of (c): one filter and one selection on the final maps, beside the round's share of the call
        for k in ("c", "c_quarter"):
            g = last[k][5]
            f = render.render_features(sc, cam, pf)
            filt = [render.reconstruct(g["raw_linear"], g["spp"] > 0, f, stderr=g["raw_stderr"], iterations=IT, want_ms=True)[4] for _ in range(args.reps)]
            sel = [render.budget_select(g["linear"], g["stderr"], g["spp"], args.cap, REL, ABS, W * H // 2, want_ms=True)[3] for _ in range(args.reps)]
            call = statistics.median(ms[k])
            print(json.dumps({"what": k + "_per_round", "scene": name, "rounds": int(g["rounds"]), "filters": int(g["rounds"]) + 1,
                              "filter_ms_median": round(statistics.median(filt), 3), "selection_ms_median": round(statistics.median(sel), 3),
                              "features_ms": round(f["stats"].kernel_ms, 3), "call_ms_per_round": round(call / max(int(g["rounds"]), 1), 3),
                              "filter_share_of_call": round(statistics.median(filt) * (int(g["rounds"]) + 1) / call, 3),
                              "spp_max": int(g["spp"].max()), "at_cap": float((g["spp"] == args.cap).mean()),
                              "valid": float(g["valid"].mean())}), flush=True)


if __name__ == "__main__":
    main()
