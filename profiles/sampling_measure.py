"""rttnw_svgf_set_sampling against the handle without it, 800x800, f64, the 16-frame orbit of 1 degree a frame on cornell_box and final_scene,
demodulate on, feedback 0.  Quality at equal cost: the handle at 4 samples a frame with boost 8 (fill 8) against the handle without sampling at a
uniform spp raised until its traced samples over the sequence are at least the boosted run's (so the uniform run never has fewer), and against the
plain 4-sample handle; MSE of the last frame against the oracle's converged t2_* windows; the samples of each run; the share of the hit pixels at
each level per frame.  Time: image_ms, stats.kernel_ms and wall time a frame (frames 1 .. 15 of the sequence, only the RGBA8 copied out) of the
boosted handle, of the same handle with sampling unset, and of a handle with sampling set at fill 1 (nothing is boosted: the probe, three list
builds and their 8-byte read-backs alone), alternating, medians of 5 runs behind a warm-up; the probe's kernel_ms beside
rttnw_temporal_accumulate's on the same frames."""
import copy, os, sys, statistics, time
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
SPP, BOOST, FILL = 4, 8, 8.0
gold = load_windows()


def sequence(sc, cams, p, sampling, want=("rgba8",), stride=1, timed=False):
    """One handle over the orbit: per frame (outputs, stats, the map or None, wall seconds)."""
    out = []
    with render.SvgfSequence(W, H, demodulate=True) as seq:
        if sampling is not None:
            seq.set_sampling(boost=sampling[0], fill=sampling[1])
        for k, c in enumerate(cams):
            pk = copy.copy(p); pk.sample_begin = k * stride * p.spp
            t0 = time.perf_counter()
            got = seq.frame(sc, c, pk, want=want)
            wall = time.perf_counter() - t0
            out.append((got, got["stats"], None if timed or sampling is None else seq.samples()[0], wall))
    return out


for name in ("cornell_box", "final_scene"):
    sc, setup = S.build(gpu, lib, name, S.load_earth() if name == "final_scene" else None)
    cam, p = S.params_for(setup, W, H, SPP, precision=abi.F64)
    cams = render.orbit_cameras(cam, FRAMES, 1.0)
    npx = W * H

    # ---- quality at equal cost
    want = ("linear_rgb", "alpha")
    boosted = sequence(sc, cams, p, (BOOST, FILL), want=want, stride=BOOST)
    feature = npx * min(SPP, 16)
    traced = sum(int(st.samples) for _, st, _, _ in boosted) - FRAMES * feature            # without the feature pass's rays
    kept = sum(int(m.sum()) for _, _, m, _ in boosted)
    uniform_spp = -(-traced // (FRAMES * npx))
    pu = copy.copy(p); pu.spp = uniform_spp
    uniform = sequence(sc, cams, pu, None, want=want)
    plain = sequence(sc, cams, p, None, want=want)
    traced_u = sum(int(st.samples) for _, st, _, _ in uniform) - FRAMES * npx * min(uniform_spp, 16)
    print("%s samples over %d frames: boosted %d traced (%d kept in the frames, %d of the plain pass discarded), %.2f a pixel and frame; uniform spp %d: %d traced; "
          "plain spp %d: %d; feature rays beside them: %d, %d, %d" % (name, FRAMES, traced, kept, traced - kept, traced / float(FRAMES * npx), uniform_spp, traced_u,
                                                                   SPP, FRAMES * npx * SPP, FRAMES * feature, FRAMES * npx * min(uniform_spp, 16), FRAMES * feature), flush=True)
    assert traced_u >= traced
    for k, (got, st, m, _) in enumerate(boosted):
        hit = got["alpha"] != 0.0
        levels = m[hit] // SPP
        print("%s frame %2d: %.1f %% of the pixels hit; of those at level 1 / 2 / 4 / 8: %s %%; %.2f samples a pixel" %
              (name, k, 100.0 * hit.mean(), " / ".join("%.1f" % (100.0 * (levels == lv).mean()) for lv in (1, 2, 4, 8)), m.mean()), flush=True)
    images = {"plain spp %d" % SPP: plain[-1][0]["linear_rgb"], "boost %d fill %g at spp %d" % (BOOST, FILL, SPP): boosted[-1][0]["linear_rgb"],
              "uniform spp %d" % uniform_spp: uniform[-1][0]["linear_rgb"]}
    for key, scene, w, h, spp, x0, y0, cw, ch, _ in WINDOWS:
        if scene != name or not key.startswith("t2_"):
            continue
        ref = gold[key + "_linear"]
        crop = (slice(y0, y0 + ch), slice(x0, x0 + cw))
        print("%s MSE: %s" % (key, "; ".join("%s %.4g" % (k, float(np.mean((v[crop] - ref) ** 2))) for k, v in images.items())), flush=True)

    # ---- time
    handles = {"sampling unset": None, "boost %d fill %g" % (BOOST, FILL): (BOOST, FILL), "boost %d fill 1 (nothing boosted)" % BOOST: (BOOST, 1.0)}
    series = {k: {"image_ms": [], "kernel_ms": [], "wall_ms": []} for k in handles}
    for k, a in handles.items(): sequence(sc, cams, p, a, timed=True)       # warm-up of every shape
    for _ in range(REPS):                                                   # alternating
        for k, a in handles.items():
            run = sequence(sc, cams, p, a, timed=True, stride=BOOST)[1:]
            series[k]["image_ms"].append(statistics.median(got["image_ms"] for got, _, _, _ in run))
            series[k]["kernel_ms"].append(statistics.median(st.kernel_ms for _, st, _, _ in run))
            series[k]["wall_ms"].append(statistics.median(1e3 * wall for _, _, _, wall in run))
    for k in handles:
        print("%s f64 800x800 handle, %-34s a frame (median of frames 1 .. 15; median of %d runs, min, max): %s" %
              (name, k, REPS, "; ".join("%s %.3f (%.3f %.3f)" % (q, statistics.median(v), min(v), max(v)) for q, v in series[k].items())), flush=True)

    # ---- the probe's kernel beside rttnw_temporal_accumulate's
    frames = []
    for k, c in enumerate(cams[-3:]):
        pk = copy.copy(p); pk.sample_begin = k * p.spp
        frames.append((render.render_host(sc, c, pk)[0], render.render_features(sc, c, pk), c))
    history = None
    for lin, f, c in frames[:2]:
        history = render.temporal_accumulate(lin, f, c, history=history)
    lin, f, c = frames[2]
    runs = {"temporal_accumulate, no history": lambda: render.temporal_accumulate(lin, f, c, want_ms=True)["ms"],
            "temporal_probe,      no history": lambda: render.temporal_probe(f, c, want_ms=True)["ms"],
            "temporal_accumulate, 1 degree on": lambda: render.temporal_accumulate(lin, f, c, history=history, want_ms=True)["ms"],
            "temporal_probe,      1 degree on": lambda: render.temporal_probe(f, c, history=history, want_ms=True)["ms"]}
    ms = {k: [] for k in runs}
    for k in runs: runs[k]()
    for _ in range(7):
        for k in runs: ms[k].append(runs[k]())
    for k in runs:
        print("%s f64 800x800 %-34s kernel_ms median %.3f (min %.3f max %.3f)" % (name, k, statistics.median(ms[k]), min(ms[k]), max(ms[k])), flush=True)
