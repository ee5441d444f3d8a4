"""The SVGF loop on the device against the host composition, 800x800, 4 samples a frame, a 16-frame orbit of 1 degree a frame on cornell_box and
final_scene.  Cost: wall time per frame and image_ms of render_sequence_device with feedback 0 and no demodulation — whose images are
render_sequence(variance=True, denoise=True)'s bit for bit (tests/test_gpu_svgf.py), so this is cost alone — against that function's wall time per
frame: medians of 5 alternating sequences behind a warm-up one; the device chain once more asking for rgba8 alone.  Quality: MSE of the last
frame against the oracle's converged t2_* windows for feedback 0 / 1 crossed with demodulate off / on, beside the host composition's."""
import os, sys, statistics, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from golden_cases import WINDOWS, load_windows
from rttnw_amd import abi, library, render
from rttnw_amd import scene as S

gpu = library.product()
lib = library.scenes()
REPS, FRAMES = 5, 16
W = H = 800
gold = load_windows()
for name in ("cornell_box", "final_scene"):
    sc, setup = S.build(gpu, lib, name, S.load_earth() if name == "final_scene" else None)
    cam, p = S.params_for(setup, W, H, 4, precision=abi.F64)
    cams = render.orbit_cameras(cam, FRAMES, 1.0)

    def timed(fn):
        t0 = time.perf_counter()
        frames = fn()
        return (time.perf_counter() - t0) * 1e3 / FRAMES, frames

    runs = {"host composition: render_sequence(variance, denoise)": lambda: render.render_sequence(sc, cams, p, variance=True, denoise=True),
            "device chain: render_sequence_device, every output": lambda: render.render_sequence_device(sc, cams, p),
            "device chain: render_sequence_device, rgba8 alone": lambda: render.render_sequence_device(sc, cams, p, want=("rgba8",))}
    ms, last = {k: [] for k in runs}, {}
    for k in runs: last[k] = runs[k]()                 # warm-up of every shape
    for _ in range(REPS):                              # alternating
        for k in runs:
            t, last[k] = timed(runs[k])
            ms[k].append(t)
    host, dev = last["host composition: render_sequence(variance, denoise)"], last["device chain: render_sequence_device, every output"]
    assert all(np.array_equal(a["rgba8"], b["rgba8"]) for a, b in zip(host, dev))
    for k in runs:
        print("%s f64 800x800 spp 4 %-58s wall ms a frame median %.2f (min %.2f max %.2f)" % (name, k, statistics.median(ms[k]), min(ms[k]), max(ms[k])),
              flush=True)
    print("%s: image_ms a frame (device time behind the trace and the feature pass) median %.3f; trace kernel_ms a frame median %.2f"
          % (name, statistics.median(f["image_ms"] for f in dev[1:]), statistics.median(f["stats"].kernel_ms for f in dev)), flush=True)
    images = {"host composition": host[-1]["linear"]}
    for feedback in (0, 1):
        for demodulate in (False, True):
            images["feedback %d, %s" % (feedback, "albedo" if demodulate else "colour")] = render.render_sequence_device(
                sc, cams, p, feedback=feedback, demodulate=demodulate, want=("linear_rgb",))[-1]["linear"]
    for key, scene, w, h, spp, x0, y0, cw, ch, _ in WINDOWS:
        if scene != name or not key.startswith("t2_"):
            continue
        ref = gold[key + "_linear"]
        crop = (slice(y0, y0 + ch), slice(x0, x0 + cw))
        print("%s MSE: %s" % (key, "; ".join("%s %.4g" % (k, float(np.mean((v[crop] - ref) ** 2))) for k, v in images.items())), flush=True)
