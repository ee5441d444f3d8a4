"""kernel_ms of rttnw_temporal_variance (both kernels) at 800x800 — the first call of a sequence (no history: every pixel that hit takes the
spatial window), the second call one degree on (a history of two frames: still every pixel spatial, and the four taps of stage A), the same
at radius 4, and the sixth call of a running sequence one degree a frame (most histories trusted: few blocks stage a tile) — beside
rttnw_temporal_accumulate over the same two frames and rttnw_denoise with five passes, without and with the estimated variance, on cornell_box
and final_scene: medians of 7 alternating runs behind a warm-up.  Then the bytes a pixel and the bandwidth they amount to."""
import copy, os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from rttnw_amd import abi, library, render
from rttnw_amd import scene as S

gpu = library.product()
lib = library.scenes()
REPS = 7
W = H = 800
for name in ("cornell_box", "final_scene"):
    sc, setup = S.build(gpu, lib, name, S.load_earth() if name == "final_scene" else None)
    cam, p = S.params_for(setup, W, H, 4, precision=abi.F64)
    cams = render.orbit_cameras(cam, 6, 1.0)
    frames = []
    for k, c in enumerate(cams):
        pk = copy.copy(p); pk.sample_begin = k * p.spp
        frames.append((render.render_host(sc, c, pk)[0], render.render_features(sc, c, pk), c))
    history, chain = None, []
    for lin, f, c in frames[:5]:
        history = render.temporal_variance(lin, f, c, history=history)
        chain.append(history)
    lin, f, c = frames[5]
    first = render.temporal_variance(*frames[4])                       # frame 4 as the start of a sequence: the history of "one degree on"
    plain_first = render.temporal_accumulate(*frames[4])
    running = render.temporal_variance(lin, f, c, history=history)
    runs = {"rttnw_denoise 5 passes": lambda: render.denoise(lin, f, None, want_ms=True)[3],
            "rttnw_denoise 5 passes, variance": lambda: render.denoise(running["linear"], f, None, want_ms=True, variance=running["variance"])[3],
            "temporal_accumulate, no history": lambda: render.temporal_accumulate(lin, f, c, want_ms=True)["ms"],
            "temporal_accumulate, 1 degree on": lambda: render.temporal_accumulate(lin, f, c, history=plain_first, want_ms=True)["ms"],
            "temporal_variance, no history": lambda: render.temporal_variance(lin, f, c, want_ms=True)["ms"],
            "temporal_variance, no history, radius 4": lambda: render.temporal_variance(lin, f, c, radius=4, want_ms=True)["ms"],
            "temporal_variance, no history, radius 1": lambda: render.temporal_variance(lin, f, c, radius=1, want_ms=True)["ms"],
            "temporal_variance, 1 degree on, 2nd frame": lambda: render.temporal_variance(lin, f, c, history=first, want_ms=True)["ms"],
            "temporal_variance, 1 degree on, running": lambda: render.temporal_variance(lin, f, c, history=history, want_ms=True)["ms"]}
    ms = {k: [] for k in runs}
    for k in runs: runs[k]()                      # warm-up of every shape
    for _ in range(REPS):                         # alternating
        for k in runs: ms[k].append(runs[k]())
    med = {k: statistics.median(ms[k]) for k in runs}
    for k in runs:
        print("%s f64 800x800 %-45s kernel_ms median %.3f (min %.3f max %.3f)" % (name, k, med[k], min(ms[k]), max(ms[k])), flush=True)
    hit = f["alpha"] != 0.0
    spatial = hit & (running["length"] < 4.0)
    # the blocks of 64 x 4 pixels that stage a tile in the running call
    blocks = spatial[: H // 4 * 4].reshape(H // 4, 4, -1)
    pad = (-W) % 64
    blocks = np.pad(blocks, ((0, 0), (0, 0), (0, pad))).reshape(H // 4, 4, -1, 64).any(axis=(1, 3))
    print("%s: running sequence, %.1f %% of the pixels hit, %.1f %% of those take the spatial estimate, %.1f %% of the blocks stage a tile"
          % (name, 100.0 * hit.mean(), 100.0 * spatial.sum() / hit.sum(), 100.0 * blocks.mean()), flush=True)
    # bytes a pixel.  Stage A: this frame 64 (colour, normal, depth, alpha), one tap's worth of the history new to the caches 96 (colour, moment,
    # length, normal, depth, alpha), written 76 (colour, moment, length, two coordinates, RGBA8).  Stage B: 64 read on the temporal branch (two
    # moments, length, alpha) and 24 written; a block that stages reads its tile instead, 88 bytes for each of (64 + 2r)(4 + 2r) pixels.
    tile = lambda r: 88.0 * (64 + 2 * r) * (4 + 2 * r) / 256.0
    a_none, a_hist = 64 + 76, 64 + 96 + 76
    for key, a, b in (("temporal_variance, no history", a_none, 16 + tile(3) + 24), ("temporal_variance, no history, radius 4", a_none, 16 + tile(4) + 24),
                      ("temporal_variance, 1 degree on, 2nd frame", a_hist, 16 + tile(3) + 24),
                      ("temporal_variance, 1 degree on, running", a_hist, 64 + 24 + blocks.mean() * tile(3))):
        print("%s: %-45s %.0f + %.0f bytes a pixel, %.0f MB, %.2f TB/s" % (name, key, a, b, (a + b) * W * H / 1e6, (a + b) * W * H / (med[key] * 1e-3) / 1e12),
              flush=True)
