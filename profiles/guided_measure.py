#!/usr/bin/env python3
"""Filter-guided adaptive sampling, measured (DESIGN.md section 10a "filter-guided form", profiles/LEDGER.md).

cornell_box and final_scene at 800x800, cap 1024, B = 64, rel_error 0.02, f64, 5 denoise iterations, three ways to the same kind of image:
  a  rttnw_render_adaptive_denoised: rounds and filter alternate on the device;
  b  rttnw_render_adaptive, then rttnw_denoise once: what `--noise 0.02 --denoise` does;
  c  the composition that defines (a), driven from Python: per round rttnw_render_adaptive_region over the mask of active pixels,
     rttnw_denoise, the stopping rule in numpy — entry points that exist without (a), so `--root` may name a checkout of the parent commit.
Per run: samples traced, device time, wall time, and the MSE of the final image against the committed oracle windows of that frame
(tests/golden/golden_windows.npz, t2_cornell_* / t2_final_*); one JSON line each.  Every run is preceded by a small call of the same kind
(scene upload, first allocations).

  python profiles/guided_measure.py [--root CHECKOUT] [--what a,b,c] [--scenes cornell_box,final_scene] [--size 800] [--cap 1024]
"""
import argparse
import copy
import hashlib
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE, help="the checkout whose package and library are measured")
    ap.add_argument("--what", default="a,b,c")
    ap.add_argument("--scenes", default="cornell_box,final_scene")
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--cap", type=int, default=1024)
    ap.add_argument("--pass-spp", type=int, default=64)
    ap.add_argument("--rel", type=float, default=0.02)
    ap.add_argument("--iterations", type=int, default=5)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import numpy as np
    from rttnw_amd import abi, library, render
    from rttnw_amd import scene as S
    from golden_cases import WINDOWS, load_windows

    gpu = library.product()
    lib = library.scenes()
    gold = load_windows()
    B, rel = args.pass_spp, args.rel

    def window_mse(name, image):
        out = {}
        for key, scene, w, h, spp, x0, y0, cw, ch, _ in WINDOWS:
            if scene == name and key.startswith("t2_") and w == args.size and h == args.size:
                out[key] = float(np.mean((image[y0:y0 + ch, x0:x0 + cw] - gold[key + "_linear"]) ** 2))
        return out

    def run_a(sc, cam, p):
        g = render.render_adaptive_denoised(sc, cam, p, B, rel, 0.0, iterations=args.iterations, want_state=False)
        return g["linear"], g["raw_linear"], g["stats"].samples, g["stats"].kernel_ms, g["rounds"]

    def run_b(sc, cam, p):
        lin, _, spp, se, st = render.render_adaptive(sc, cam, p, B, rel, 0.0)
        pf = copy.copy(p)
        pf.spp = B
        f = render.render_features(sc, cam, pf)
        out, _, _, ms = render.denoise(lin, f, se, iterations=args.iterations, want_ms=True)
        return out, lin, st.samples, st.kernel_ms + f["stats"].kernel_ms + ms, int(spp.max()) // B

    def run_c(sc, cam, p):
        h, w = p.height, p.width
        pf = copy.copy(p)
        pf.spp = B
        f = render.render_features(sc, cam, pf)
        ms, samples, rounds = f["stats"].kernel_ms, 0, 0
        active = np.ones((h, w), dtype=bool)
        state = None
        for k in range(p.spp // B):
            if not active.any():
                break
            pk = copy.copy(p)
            pk.spp = (k + 1) * B
            lin, _, spp, se, st, state = render.render_adaptive_region(sc, cam, pk, 0, 0, w, h, mask=active, state=state, pass_spp=B,
                                                                      rel_error=0.0, abs_error=0.0)
            den, _, var_f, dms = render.denoise(lin, f, se, iterations=args.iterations, want_ms=True)
            with np.errstate(invalid="ignore"):
                filtered = (np.isfinite(var_f) & (np.sqrt(var_f) <= rel * den)).all(axis=2)
            active &= ~((se == 0.0).all(axis=2) | filtered)
            ms += st.kernel_ms + dms
            samples += st.samples
            rounds += 1
        return den, lin, samples, ms, rounds

    runs = {"a": run_a, "b": run_b, "c": run_c}
    for name in args.scenes.split(","):
        sc, setup = S.build(gpu, lib, name, S.load_earth() if name == "final_scene" else None)
        cam, p = S.params_for(setup, args.size, args.size, args.cap, precision=abi.F64)
        cam_s, p_s = S.params_for(setup, 64, 64, 2 * B, precision=abi.F64)
        for what in args.what.split(","):
            runs[what](sc, cam_s, p_s)
            t0 = time.time()
            image, raw, samples, ms, rounds = runs[what](sc, cam, p)
            wall = time.time() - t0
            print(json.dumps({"what": what, "scene": name, "size": args.size, "cap": args.cap, "pass_spp": B, "rel_error": rel, "rounds": rounds,
                              "samples": int(samples), "of": args.size * args.size * args.cap, "kernel_ms": round(ms, 2), "wall_s": round(wall, 3),
                              "mse": window_mse(name, image), "mse_raw": window_mse(name, raw),
                              "image_sha1": hashlib.sha1(np.ascontiguousarray(image).tobytes()).hexdigest()[:12]}), flush=True)


if __name__ == "__main__":
    main()
