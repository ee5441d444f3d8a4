"""`python -m rttnw_amd <scene>` — the reference's CLI (src/main.rs:236-258) on the HIP path.

One positional argument, the scene number 1..9 with the reference's per-scene defaults (size, spp, camera:
main.rs:66-183); writes `image.png` into the current directory (main.rs:231) and prints the wall time.
Optional extras (not in the reference): --spp, --width, --precision f32|f64, --out, --seed, --passes, and adaptive sampling:
--noise R [--abs-noise A] [--pass-spp B] [--spp-map FILE] stops sampling a pixel once the standard error of its mean is at most
A + R * mean in every channel, --spp being the cap.  --denoise [--denoise-iterations N] filters the image with rttnw_denoise, guided by
first-hit feature buffers of min(spp, 16) samples (and, with --noise, by the adaptive render's standard errors); --features PREFIX writes
PREFIX_albedo.png, PREFIX_normal.png (n * 0.5 + 0.5), PREFIX_depth.png (normalised to the farthest hit) and PREFIX_alpha.png.
--window X0,Y0,X1,Y1 renders pixels [X0, X1) x [Y0, Y1) of the frame only (rttnw_render_region) and writes that window as the image; it does
not combine with --noise, --denoise, --features or --passes.
--devices 0,1,2,... renders on those GPUs of the node (a device may repeat: logical ranks on one GPU): rttnw_render_multi, or with --noise
rttnw_render_adaptive_multi — the same image either way.  It does not combine with --window, --features, --denoise or --passes.
--save-state FILE and --resume FILE (with --noise only; they combine with --devices): the adaptive render leaves its state — the double array of
rttnw_render_adaptive_resume, as .npy — in FILE, and starts from the state in FILE: a preview refined under a tighter --noise or a higher --spp
without retracing a sample, on the same scene, size, seed and --pass-spp.  They do not combine with --window or --passes.
--refine X0,Y0,X1,Y1 (with --noise only) brings pixels [X0, X1) x [Y0, Y1) of the frame to the noise bound (rttnw_render_adaptive_region) and writes
that window as the image: alone it samples the window from nothing; with --resume it starts from the state in FILE — a preview's noisy patch refined
where one looks, the rest of the state untouched — and --save-state leaves the frame-sized state, in which pixels never sampled are zero records.  It
combines with --spp, --pass-spp, --devices and --spp-map, and not with --window, --passes, --features or --denoise.
--guided (with --noise only) stops pixels on the noise of the FILTERED image (rttnw_render_adaptive_denoised): the adaptive rounds and the denoiser
alternate on the device, --denoise-iterations sets its passes, the image written is the denoised one (--denoise is implied), --spp-map and
--save-state work as before, and the samples traced and the rounds run are printed.  It does not combine with --devices, --resume, --refine,
--window or --passes.
--preview L (with --noise only; L = 0 .. 6) traces only the pixels with x % 2^L == 0 and y % 2^L == 0, 1 in 4^L, and reconstructs the frame from them
(rttnw_render_preview): the image written is the reconstruction, --denoise-iterations sets its passes, --spp-map shows the lattice, and --save-state
leaves the frame-sized state with zero records off the lattice — `--resume state.npy --refine 0,0,W,H` then completes the frame without retracing
a sample.  It does not combine with --devices, --resume, --refine, --guided, --window or --passes.
--budget SAMPLES (with --noise only) traces at most SAMPLES camera paths and spends them on the noisiest pixels first (rttnw_render_adaptive_budget):
rounds that give one more pass to the pixels furthest above the noise bound, --spp being the cap; pixels the budget never reached stay black.  It
works with --resume, --save-state and --spp-map, prints the samples traced and the rounds run, and does not combine with --preview, --guided,
--refine, --devices, --window or --passes.
--guided-budget SAMPLES (with --noise only) is --budget ranked by the noise of the FILTERED image (rttnw_render_adaptive_budget_denoised): each round
filters the frame on the device and gives one more pass to the pixels whose filtered value stands furthest above the noise bound; the image
written is the filtered one, --denoise-iterations sets its passes, and a pixel nothing could be filled into stays transparent.  It works with
--resume, --save-state and --spp-map, prints the samples traced and the rounds run, and does not combine with --budget, --guided, --preview,
--refine, --devices, --window or --passes.
--denoise-nlm [--nlm-search-radius R] [--nlm-patch-radius F] [--nlm-k K] renders the frame as two halves of spp / 2 samples over disjoint sample
ranges and filters them with rttnw_denoise_nlm, non-local means whose weights for one half are measured in the other: no feature buffer, so what a
mirror shows or a texture paints is filtered like anything else.  --spp must be even.  It does not combine with --noise, --denoise, --features,
--devices, --window or --passes.
--denoise-select [--select-margin X] [--blend-map FILE] renders the same two halves and the first-hit features of min(spp, 16) samples, filters
each half with rttnw_denoise and with non-local means, and takes per pixel the filter that lies closer to the other, raw half
(rttnw_denoise_select): walls go to the feature-guided filter, textures and reflections to non-local means.  X is the margin non-local means
must win by (-2 .. 2; without the flag the library default, 0.01); FILE receives the blend weight as a grey PNG (white: non-local means).
--denoise-iterations and the --nlm- flags set the two filters.  --spp must be even.  It does not combine with --noise, --denoise,
--denoise-nlm, --features, --devices, --window or --passes.
--denoise-regress [--ridge X] [--regress-features anz] [--no-demodulate] [--fit-map FILE] renders the same two halves and the first-hit features of
min(spp, 16) samples and fits, per pixel, a linear model of colour in the features under non-local means' weights, keeping its intercept
(rttnw_denoise_regress): what the features explain — a texture, a shading gradient, a depth ramp — is not blurred.  --regress-features takes the
letters of the regressors (a albedo, n normal, z depth; default anz; "none" for no regressor), X is the ridge (0: the library default),
--no-demodulate filters colour in place of colour / albedo, FILE receives the fit count as a grey PNG (white: both directions used the first-order
fit).  The --nlm- flags set the weights.  --spp must be even.  It does not combine with --noise, --denoise, --denoise-nlm, --denoise-select,
--features, --devices, --window or --passes.
--orbit K [--orbit-step DEG] [--temporal] [--denoise] renders K frames of --spp samples each from a camera that turns about the axis through
lookat along view_up, DEG degrees a frame (default 1.0), and ENDS at the scene's own camera: frame k's lookfrom is the scene's, turned by
(k - (K - 1)) * DEG degrees.  Frame k takes its samples at sample_begin = k * spp, so the frames are independent estimates.  With --temporal
every frame is blended with the previous result, fetched from where each pixel's surface point was in the previous frame
(rttnw_temporal_accumulate, guided by first-hit features of min(spp, 16) samples); with --denoise the frame written is rttnw_denoise of it,
and the history stays unfiltered.  The frames are written as frame_000.png, frame_001.png, ... beside --out.  --orbit does not combine with
--noise, --window, --devices, --denoise-nlm, --denoise-select, --denoise-regress, --features or --passes; --temporal needs --orbit.
--temporal-variance (it implies --temporal and needs --orbit) carries the colour's second moment along the same history and estimates the
variance of every pixel's accumulated mean (rttnw_temporal_variance: from the two moments where the history counts 4 frames, from a 7x7 window
guided by normal and depth elsewhere); with --denoise that variance is rttnw_denoise's colour stop: accumulate, estimate, filter.
--svgf [--feedback J] [--demodulate] (it needs --orbit) runs that whole loop on the device, the history never leaving it (rttnw_svgf_frame):
the frames of --orbit K --temporal-variance --denoise, bit for bit, without the copies between the stages.  --feedback J feeds the filter's
result after J passes (0 .. --denoise-iterations; SVGF: 1) back into the colour history; --demodulate accumulates, estimates and filters
colour / albedo, so textures neither blur in the reprojection nor read as variance.  --feedback and --demodulate need --svgf.
--clamp GAMMA (with --temporal-variance or --svgf) clips the reprojected history to each frame before the blend (rttnw_temporal_clamp): the mean
and the standard deviation of the frame's colour over a 7x7 window guided by normal and depth admit the history within GAMMA deviations (0: the
default, 1.0) and move it to the nearer bound outside — ghosts of reflections and refractions go, at the price of some noise coming back.
--boost B (with --svgf; 1, 2, 4 or 8) gives pixels whose reprojected history is thin — disocclusions, the frame's edge, the first frame — up to B
times --spp samples in that frame (rttnw_svgf_set_sampling): the largest of 1, 2, 4, 8 that is at most B and at most FILL / (history length + 1),
--fill FILL (default 8).  --spp-map spp_%03d.png writes each frame's samples per pixel as a grey image (spp * 255 / (B * --spp)).
--spatial nlm|regress (with --svgf; an even --spp) replaces the loop's à-trous filter by rttnw_denoise_nlm or rttnw_denoise_regress over two half
histories the handle accumulates along the same reprojection (rttnw_svgf_set_regress): the weights are measured on accumulated halves, not on
two halves of one frame.  --regress-variance temporal|pair chooses the variances those weights read: the loop's temporal estimate (the default)
or the filter's own pair variance.  --fit-map fit_%03d.png writes each frame's fit count as a grey image.  The stage does not combine with
--feedback, --clamp or --boost.
"""
import argparse
import sys
import time

import numpy as np

USAGE = """Usage: python -m rttnw_amd <scene>
Possible scenes:
\t- 1: random_scene
\t- 2: two_spheres
\t- 3: two_perlin_spheres
\t- 4: earth
\t- 5: simple_light
\t- 6: empty_cornell_box
\t- 7: cornell_box
\t- 8: smoke_cornell_box
\t- 9: final_scene"""


def parse_window(text):
    """'X0,Y0,X1,Y1' -> four non-negative integers with X0 < X1 and Y0 < Y1, or None."""
    parts = text.split(",")
    if len(parts) != 4 or not all(s.strip().isdigit() for s in parts):
        return None
    x0, y0, x1, y1 = (int(s) for s in parts)
    return (x0, y0, x1, y1) if x0 < x1 and y0 < y1 else None


def regress_mask(text):
    """'anz' -> 7: the feature mask of rttnw_denoise_regress from the letters a (albedo, 1), n (normal, 2), z (depth, 4) in any order; 'none' -> 0;
    None for another letter, a repeated one or an empty string."""
    if text == "none":
        return 0
    bits = {"a": 1, "n": 2, "z": 4}
    if not text or any(ch not in bits for ch in text) or len(set(text)) != len(text):
        return None
    return sum(bits[ch] for ch in text)


def parse_devices(text):
    """'0,1,2' -> [0, 1, 2]: 1 to 64 non-negative integers (repeats allowed), or None."""
    parts = text.split(",")
    if not 1 <= len(parts) <= 64 or not all(s.strip().isdigit() for s in parts):
        return None
    return [int(s) for s in parts]


def node_ms(devices, stats):
    """Device time of a multi-rank render: ranks that share a device run one after the other, devices side by side."""
    per_device = {}
    for dev, st in zip(devices, stats):
        per_device[dev] = per_device.get(dev, 0.0) + st.kernel_ms
    return max(per_device.values())


EVEN_SPP = "%s needs an even --spp (two halves of spp / 2 samples), got %d"
WANTS_WINDOW = "%s wants X0,Y0,X1,Y1: four non-negative integers with X0 < X1 and Y0 < Y1, got %r"


def refusal(args, refine, devices, window):
    """The first rule the flags break, as the line for stderr, or None.  `refine`, `devices` and `window` are the parsed values, None where malformed."""
    on = {"--noise": args.noise is not None, "--guided-budget": args.guided_budget is not None, "--budget": args.budget is not None,
          "--preview": args.preview is not None, "--guided": args.guided,
          "--refine": args.refine is not None, "--devices": args.devices is not None, "--resume": args.resume is not None,
          "--save-state": args.save_state is not None, "--window": args.window is not None, "--passes": args.passes > 1,
          "--features": args.features is not None, "--denoise": args.denoise, "--denoise-nlm": args.denoise_nlm,
          "--denoise-select": args.denoise_select, "--denoise-regress": args.denoise_regress, "--orbit": args.orbit is not None}
    iterations = (0 <= args.denoise_iterations <= 8, "--denoise-iterations must be 0 .. 8")
    state_needs, state_clashes = "only the adaptive render has a state", ("--window", "--passes")
    # in the order they are checked: (flag, why it needs --noise or None, the flags it does not combine with, the reason given for that,
    # [(holds, the message if not)] checked before all that, the same checked after it)
    noise_above_0 = "%s needs a noise bound above 0 to rank pixels by (--noise or --abs-noise)"
    nlm_parameters = [(0 <= args.nlm_search_radius <= 16, "--nlm-search-radius must be 0 .. 16 (0: the default, 7)"),
                      (0 <= args.nlm_patch_radius <= 4, "--nlm-patch-radius must be 0 .. 4 (0: the default, 3)"),
                      (args.nlm_k >= 0.0, "--nlm-k must be at least 0 (0: the default, 0.7)")]
    if args.blend_map is not None and not args.denoise_select:
        return "--blend-map needs --denoise-select: only that call has a blend weight"
    staged = args.svgf and args.spatial in ("nlm", "regress")   # the regression filter as the loop's spatial stage: --fit-map goes with it too
    if (args.ridge is not None or args.regress_features is not None or args.no_demodulate or (args.fit_map is not None and not staged)) and not args.denoise_regress:
        return "--ridge, --regress-features, --no-demodulate and --fit-map need --denoise-regress: only that call has them"
    if (args.spatial is not None or args.regress_variance is not None) and not args.svgf:
        return "--spatial and --regress-variance need --svgf: only the loop on the device has a choice of spatial stage"
    if args.regress_variance is not None and not staged:
        return "--regress-variance needs --spatial nlm or --spatial regress: the à-trous stage takes the temporal estimate as it is"
    if staged and (args.feedback or args.clamp is not None or args.boost is not None):
        return "--spatial %s does not combine with --feedback, --clamp or --boost: the stage is exclusive with them" % args.spatial
    if staged and args.spp and (args.spp < 2 or args.spp % 2):
        return EVEN_SPP % ("--spatial " + args.spatial, args.spp)
    if staged and args.fit_map is not None and "%" not in args.fit_map:
        return "--fit-map with --svgf names one file per frame: it needs a %d (as in fit_%03d.png)"
    if args.regress_features is not None and regress_mask(args.regress_features) is None:
        return "--regress-features wants letters of a (albedo), n (normal), z (depth), or none; got %r" % args.regress_features
    if args.svgf and not on["--orbit"]:
        return "--svgf needs --orbit: it runs the accumulate, estimate, filter loop over the frames of a sequence"
    if (args.feedback or args.demodulate) and not args.svgf:
        return "--feedback and --demodulate need --svgf: only the loop on the device has them"
    if args.clamp is not None and not (args.temporal_variance or args.svgf):
        return "--clamp needs --temporal-variance or --svgf: it clips the history those accumulate"
    if args.clamp is not None and not args.clamp >= 0.0:
        return "--clamp must be at least 0 standard deviations (0: the default, 1.0)"
    if (args.boost is not None or args.fill is not None) and not args.svgf:
        return "--boost and --fill need --svgf: only the loop on the device chooses samples per pixel"
    if args.fill is not None and args.boost is None:
        return "--fill needs --boost: without it every pixel gets --spp samples"
    if args.boost is not None and args.boost not in (1, 2, 4, 8):
        return "--boost must be 1, 2, 4 or 8"
    if args.fill is not None and not 1.0 <= args.fill < float("inf"):
        return "--fill must be finite and at least 1"
    if args.svgf and args.spp_map is not None and args.boost is None:
        return "--spp-map with --svgf needs --boost: without it every pixel gets --spp samples"
    if args.svgf and args.spp_map is not None and "%" not in args.spp_map:
        return "--spp-map with --svgf names one file per frame: it needs a %d (as in spp_%03d.png)"
    if args.temporal_variance and not on["--orbit"]:
        return "--temporal-variance needs --orbit: it estimates the variance from the accumulated frames of a sequence"
    if args.temporal and not on["--orbit"]:
        return "--temporal needs --orbit: it accumulates the frames of a sequence"
    rules = [
        ("--orbit", None, ("--noise", "--window", "--devices", "--denoise-nlm", "--denoise-select", "--denoise-regress", "--features", "--passes"),
         ": it renders a sequence of plain frames of the whole image, on one GPU", [],
         [(not on["--orbit"] or 1 <= args.orbit <= 1000, "--orbit must be 1 .. 1000 frames"),
          (args.orbit_step == args.orbit_step and abs(args.orbit_step) <= 360.0, "--orbit-step must be -360 .. 360 degrees"), iterations,
          (0 <= args.feedback <= max(args.denoise_iterations, 0), "--feedback must be 0 .. --denoise-iterations (%d)" % args.denoise_iterations)]),
        ("--denoise-select", None, ("--noise", "--denoise", "--denoise-nlm", "--features", "--devices", "--window", "--passes"),
         ": it filters two plain half renders of the whole frame with both filters, on one GPU", [],
         [(args.spp == 0 or (args.spp >= 2 and args.spp % 2 == 0), EVEN_SPP % ("--denoise-select", args.spp)),
          (args.select_margin is None or -2.0 <= args.select_margin <= 2.0, "--select-margin must be -2 .. 2 (without it: the default, 0.01)"),
          iterations] + nlm_parameters),
        ("--denoise-regress", None, ("--noise", "--denoise", "--denoise-nlm", "--denoise-select", "--features", "--devices", "--window", "--passes"),
         ": it fits two plain half renders of the whole frame to their first-hit features, on one GPU", [],
         [(args.spp == 0 or (args.spp >= 2 and args.spp % 2 == 0), EVEN_SPP % ("--denoise-regress", args.spp)),
          (args.ridge is None or args.ridge >= 0.0, "--ridge must be at least 0 (0: the library default)")] + nlm_parameters),
        ("--denoise-nlm", None, ("--noise", "--denoise", "--features", "--devices", "--window", "--passes"),
         ": it filters two plain half renders of the whole frame, on one GPU", [], nlm_parameters),
        ("--guided-budget", "it is the adaptive render under a budget of samples, ranked by the filtered image's noise",
         ("--budget", "--guided", "--preview", "--refine", "--devices", "--window", "--passes"),
         ": it runs on one GPU, over the whole frame, on the filtered noise", [],
         [(not on["--guided-budget"] or args.guided_budget >= 0, "--guided-budget must be at least 0"),
          ((args.noise or 0.0) > 0.0 or args.abs_noise > 0.0, noise_above_0 % "--guided-budget"), iterations]),
        ("--budget", "it is the adaptive render under a budget of samples", ("--preview", "--guided", "--refine", "--devices", "--window", "--passes"),
         ": it runs on one GPU, over the whole frame, on the raw noise", [],
         [(not on["--budget"] or args.budget >= 0, "--budget must be at least 0"),
          ((args.noise or 0.0) > 0.0 or args.abs_noise > 0.0, noise_above_0 % "--budget")]),
        ("--preview", "it is the adaptive render of a lattice of the frame, reconstructed",
         ("--devices", "--resume", "--refine", "--guided", "--window", "--passes"), ": it runs on one GPU, over the whole frame, from nothing", [],
         [(not on["--preview"] or 0 <= args.preview <= 6, "--preview must be 0 .. 6"), iterations]),
        ("--guided", "it is the adaptive render stopped on the filtered image's noise", ("--devices", "--resume", "--refine", "--window", "--passes"),
         ": it runs on one GPU, over the whole frame, from nothing", [], [iterations]),
        ("--refine", "it brings a window to a noise bound", ("--window", "--passes", "--features", "--denoise"),
         ": it runs the adaptive render over a window of the frame", [], [(refine is not None, WANTS_WINDOW % ("--refine", args.refine))]),
        ("--devices", None, ("--window", "--features", "--denoise", "--passes"), ": it runs the plain and the adaptive render only",
         [(devices is not None, "--devices wants D0,D1,...: 1 to 64 non-negative device numbers separated by commas, got %r" % args.devices)], []),
        ("--resume", state_needs, state_clashes, "", [], []),
        ("--save-state", state_needs, state_clashes, "", [], []),
        ("--window", None, ("--noise", "--denoise", "--features", "--passes"), ": it renders pixels of the plain frame only",
         [(window is not None, WANTS_WINDOW % ("--window", args.window))], []),
    ]
    for flag, needs_noise, clashes, why, before, after in rules:
        if not on[flag]:
            continue
        clash = [name for name in clashes if on[name]]
        for holds, message in before + [(on["--noise"] or needs_noise is None, "%s needs --noise: %s" % (flag, needs_noise)),
                                        (not clash, "%s does not combine with %s%s" % (flag, ", ".join(clash), why))] + after:
            if not holds:
                return message
    return None


def save_state(path, state):
    with open(path, "wb") as f:    # (an open file: np.save would append .npy to a bare name)
        np.save(f, state)


def load_state(path):
    """The adaptive state in `path`, or None after saying on stderr why it cannot be read."""
    try:
        return np.load(path)
    except (OSError, ValueError) as e:
        print("--resume %s: %s" % (path, e), file=sys.stderr)
        return None


def main(argv=None):
    ap = argparse.ArgumentParser(add_help=True, usage=USAGE)
    ap.add_argument("scene", type=int)
    ap.add_argument("--spp", type=int, default=0)
    ap.add_argument("--width", type=int, default=0)
    ap.add_argument("--precision", default="f64", choices=["f32", "f64", "f64strict"], help="f64 = the reference's arithmetic (default); f32 = throughput; f64strict = f64 with nothing contracted (bit-for-bit the CPU reference's path decisions)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default="image.png")
    ap.add_argument("--passes", type=int, default=1, help="render in this many passes over disjoint sample ranges, "
                    "rewriting the image after each (progressive)")
    ap.add_argument("--noise", type=float, default=None, help="adaptive sampling: relative noise bound (standard error / mean); --spp is the cap")
    ap.add_argument("--abs-noise", type=float, default=0.0, help="adaptive sampling: absolute noise bound added to the relative one")
    ap.add_argument("--pass-spp", type=int, default=64, help="adaptive sampling: samples per pixel per pass (the cap must be a multiple)")
    ap.add_argument("--spp-map", default=None, help="adaptive sampling: also write a grey-scale PNG of samples / cap; svgf with --boost: one per frame, the name holding a %%d for the frame's number, as in spp_%%03d.png")
    ap.add_argument("--denoise", action="store_true", help="filter the image with the feature-guided denoiser (rttnw_denoise)")
    ap.add_argument("--denoise-iterations", type=int, default=5, help="a-trous passes of the denoiser (0..8)")
    ap.add_argument("--denoise-nlm", action="store_true", help="render two halves of spp / 2 samples and filter them with non-local means "
                    "(rttnw_denoise_nlm): no feature buffer")
    ap.add_argument("--nlm-search-radius", type=int, default=0, help="non-local means: candidates within this many pixels (1..16; 0 = 7)")
    ap.add_argument("--nlm-patch-radius", type=int, default=0, help="non-local means: patches of (2F+1)^2 pixels (1..4; 0 = 3)")
    ap.add_argument("--nlm-k", type=float, default=0.0, help="non-local means: the distance scale (0 = 0.7)")
    ap.add_argument("--denoise-select", action="store_true", help="render two halves and the first-hit features, filter each half with both "
                    "denoisers and take per pixel the one closer to the other half (rttnw_denoise_select)")
    ap.add_argument("--select-margin", type=float, default=None, metavar="X", help="selection: the margin non-local means must win by (-2..2; "
                    "default 0.01)")
    ap.add_argument("--blend-map", default=None, metavar="FILE", help="selection: also write the blend weight as a grey-scale PNG (white: "
                    "non-local means)")
    ap.add_argument("--denoise-regress", action="store_true", help="render two halves and the first-hit features and fit colour to the features "
                    "under non-local means' weights (rttnw_denoise_regress)")
    ap.add_argument("--ridge", type=float, default=None, metavar="X", help="regression: the ridge (0 or absent: the library default)")
    ap.add_argument("--regress-features", default=None, metavar="anz", help="regression: the regressors, letters of a (albedo), n (normal), "
                    "z (depth), or none (default anz)")
    ap.add_argument("--no-demodulate", action="store_true", help="regression: filter colour, not colour / albedo")
    ap.add_argument("--fit-map", default=None, metavar="FILE", help="regression: also write the fit count as a grey-scale PNG (white: both "
                    "directions used the first-order fit)")
    ap.add_argument("--orbit", type=int, default=None, metavar="K", help="render K frames from a camera that turns about lookat and ends at the "
                    "scene's own; writes frame_000.png, ... beside --out")
    ap.add_argument("--orbit-step", type=float, default=1.0, metavar="DEG", help="orbit: degrees per frame (default 1.0)")
    ap.add_argument("--temporal", action="store_true", help="orbit: blend every frame with the reprojected previous result "
                    "(rttnw_temporal_accumulate)")
    ap.add_argument("--temporal-variance", action="store_true", help="orbit: --temporal, and estimate the variance of every pixel's accumulated "
                    "mean from the frame history (rttnw_temporal_variance); --denoise then filters with it")
    ap.add_argument("--svgf", action="store_true", help="orbit: accumulate, estimate and filter every frame on the device, the history never leaving "
                    "it (rttnw_svgf_frame)")
    ap.add_argument("--feedback", type=int, default=0, metavar="J", help="svgf: feed the filter's result after J passes back into the colour history "
                    "(0 .. --denoise-iterations; default 0: the unfiltered accumulation)")
    ap.add_argument("--demodulate", action="store_true", help="svgf: accumulate, estimate and filter colour / albedo")
    ap.add_argument("--spatial", choices=("atrous", "nlm", "regress"), default=None, help="svgf: the spatial stage — the à-trous filter (the default), "
                    "or non-local means / the first-order regression over two accumulated halves (rttnw_svgf_set_regress; an even --spp)")
    ap.add_argument("--regress-variance", choices=("temporal", "pair"), default=None, help="svgf, with --spatial nlm or regress: the variances the "
                    "filter's weights read — the loop's temporal estimate (the default) or the filter's own pair variance")
    ap.add_argument("--clamp", type=float, default=None, metavar="GAMMA", help="temporal-variance, svgf: clip the reprojected history into the frame's "
                    "neighbourhood mean +- GAMMA standard deviations before the blend (rttnw_temporal_clamp; 0: the default, 1.0)")
    ap.add_argument("--boost", type=int, default=None, metavar="B", help="svgf: up to B (1, 2, 4 or 8) times --spp samples for pixels whose reprojected "
                    "history is thin (rttnw_svgf_set_sampling)")
    ap.add_argument("--fill", type=float, default=None, metavar="FILL", help="svgf, with --boost: a pixel is boosted while (history length + 1) * "
                    "multiplier <= FILL (default 8)")
    ap.add_argument("--guided", action="store_true", help="adaptive sampling: stop pixels on the noise of the denoised image "
                    "(rttnw_render_adaptive_denoised); writes the denoised image")
    ap.add_argument("--preview", type=int, default=None, metavar="L", help="adaptive sampling: trace 1 pixel in 4^L (x %% 2^L == 0 and y %% 2^L == 0, "
                    "L = 0 .. 6) and reconstruct the frame from them (rttnw_render_preview); writes the reconstruction")
    ap.add_argument("--budget", type=int, default=None, metavar="SAMPLES", help="adaptive sampling: trace at most SAMPLES camera paths, the noisiest "
                    "pixels first (rttnw_render_adaptive_budget)")
    ap.add_argument("--guided-budget", type=int, default=None, metavar="SAMPLES", help="adaptive sampling: trace at most SAMPLES camera paths, the "
                    "pixels whose DENOISED value is noisiest first (rttnw_render_adaptive_budget_denoised); writes the filtered image")
    ap.add_argument("--features", default=None, metavar="PREFIX", help="write the first-hit feature buffers as PREFIX_albedo.png, "
                    "PREFIX_normal.png, PREFIX_depth.png, PREFIX_alpha.png")
    ap.add_argument("--window", default=None, metavar="X0,Y0,X1,Y1", help="render pixels [X0, X1) x [Y0, Y1) of the frame only (row 0 = top) "
                    "and write that window as the image")
    ap.add_argument("--refine", default=None, metavar="X0,Y0,X1,Y1", help="adaptive sampling: bring pixels [X0, X1) x [Y0, Y1) of the frame to the "
                    "noise bound, from the --resume state if given, and write that window as the image")
    ap.add_argument("--devices", default=None, metavar="D0,D1,...", help="render on these GPUs of the node (repeats allowed: logical ranks); "
                    "with --noise the adaptive render runs across them")
    ap.add_argument("--save-state", default=None, metavar="FILE", help="adaptive sampling: leave the render's state in FILE (.npy) for a later --resume")
    ap.add_argument("--resume", default=None, metavar="FILE", help="adaptive sampling: start from the state in FILE instead of from nothing")
    try:
        args = ap.parse_args(argv)
    except SystemExit:
        print("There was an error", file=sys.stderr)   # DummyError, main.rs:260-268
        raise
    refine = parse_window(args.refine) if args.refine is not None else None
    devices = parse_devices(args.devices) if args.devices is not None else None
    window = parse_window(args.window) if args.window is not None else None
    refused = refusal(args, refine, devices, window)
    if refused:
        print(refused, file=sys.stderr)
        return 1
    args.temporal = args.temporal or args.temporal_variance
    from PIL import Image
    from . import abi, library, render
    from .abi import CameraDesc
    from .scene import Scene, load_earth, make_params

    scenes = library.scenes()
    name = scenes.scenes_name(args.scene)
    if not name:
        print("There is no scene %d" % args.scene, file=sys.stderr)   # main.rs:179-182
        return 1
    print("Scene number: %d" % args.scene)
    print("Running scene %s" % name.decode())
    t0 = time.time()
    sc = Scene(library.product(), scenes_binding=scenes)
    setup = sc.build_named(name.decode(), earth_rgba=load_earth())
    w = args.width or setup.width
    h = int(w / (setup.width / setup.height))                        # height = (width / aspect) as u32, main.rs:184
    cam = CameraDesc.from_buffer_copy(setup.camera)
    cam.aspect_ratio = setup.width / setup.height
    p = make_params(w, h, args.spp or setup.spp, background=tuple(setup.background), seed=args.seed,
                    precision={"f32": abi.F32, "f64": abi.F64, "f64strict": abi.F64_STRICT}[args.precision])
    staged = args.svgf and args.spatial in ("nlm", "regress")
    for flag, on in (("--denoise-select", args.denoise_select), ("--denoise-regress", args.denoise_regress), ("--spatial %s" % args.spatial, staged)):
        if on and (p.spp < 2 or p.spp % 2):   # (the scene's own spp: a given --spp was refused above)
            print(EVEN_SPP % (flag, p.spp), file=sys.stderr)
            return 1
    if window is not None:
        x0, y0, x1, y1 = window
        if x1 > w or y1 > h:
            print("--window %s reaches outside the %dx%d frame" % (args.window, w, h), file=sys.stderr)
            return 1
        _, rgba, st = render.render_region(sc, cam, p, x0, y0, x1, y1)
        Image.fromarray(np.ascontiguousarray(rgba), "RGBA").save(args.out)
        print("%.3fs (window %dx%d at (%d, %d) of %dx%d: %d samples, kernels %.1f ms)"
              % (time.time() - t0, x1 - x0, y1 - y0, x0, y0, w, h, st.samples, st.kernel_ms))
        return 0
    if args.orbit is not None:
        import os
        where = os.path.dirname(args.out) or "."
        trace_ms = [0.0]

        def write(k, frame):
            trace_ms[0] += frame["stats"].kernel_ms
            Image.fromarray(np.ascontiguousarray(frame["rgba8"]), "RGBA").save(os.path.join(where, "frame_%03d.png" % k))
            if args.svgf and args.spp_map is not None:
                grey = (frame["spp"].astype(np.uint64) * 255 // (args.boost * p.spp)).astype(np.uint8)
                Image.fromarray(grey, "L").save(args.spp_map % k)
            if staged and args.fit_map is not None:
                Image.fromarray((frame["halves"]["fit"] * 127.5).astype(np.uint8), "L").save(args.fit_map % k)

        if args.svgf:
            frames = render.render_sequence_device(sc, render.orbit_cameras(cam, args.orbit, args.orbit_step), p, feedback=args.feedback,
                                                   demodulate=args.demodulate, iterations=args.denoise_iterations, on_frame=write, clamp=args.clamp,
                                                   sampling=None if args.boost is None else (args.boost, args.fill or 0.0),
                                                   want_spp=args.boost is not None, spatial=args.spatial or "atrous",
                                                   regress_variance=args.regress_variance or "temporal", want_halves=staged and args.fit_map is not None)
            args.temporal = args.temporal_variance = True
        else:
            frames = render.render_sequence(sc, render.orbit_cameras(cam, args.orbit, args.orbit_step), p, temporal=args.temporal, denoise=args.denoise,
                                            iterations=args.denoise_iterations, on_frame=write, variance=args.temporal_variance, clamp=args.clamp)
        clamped = "" if args.clamp is None else ", the history clipped at gamma %g" % (args.clamp or 1.0)
        print("%.3fs (%d frames of %d spp, %g degrees apart%s: trace kernels %.1f ms; written to %s)"
              % (time.time() - t0, args.orbit, p.spp, args.orbit_step, clamped, trace_ms[0], os.path.join(where, "frame_000.png ...")))
        if args.temporal:
            length = frames[-1]["length"]
            print("temporal: the last frame's history counts %.2f frames on average, %.1f %% of its pixels were reset"
                  % (length.mean(), 100.0 * (length == 1.0).mean() if args.orbit > 1 else 0.0))
        if args.svgf and args.boost is not None:
            total = sum(int(f["spp"].sum()) for f in frames)
            print("sampling: boost %d, fill %g: %.2f samples a pixel and frame on average (%d traced in all, the feature pass's rays and the plain pass's discarded samples included)"
                  % (args.boost, args.fill or 8.0, total / (len(frames) * float(w * h)),
                     sum(int(f["stats"].samples) for f in frames)))
        if args.svgf:
            print("svgf: feedback %d, %s; %.3f ms a frame on the device behind the trace and the feature pass"
                  % (args.feedback, "colour / albedo" if args.demodulate else "colour", sum(f["image_ms"] for f in frames) / len(frames)))
        if staged:
            print("spatial stage: %s over two accumulated halves, its weights on the %s variance"
                  % ("first-order regression" if args.spatial == "regress" else "non-local means", args.regress_variance or "temporal"))
        if args.temporal_variance:
            var = frames[-1]["accumulated"]["variance"]
            print("temporal-variance: the last frame's mean standard error is %.4g; %.1f %% of its pixels took the spatial estimate"
                  % (np.sqrt(var).mean(), 100.0 * ((length < 4.0) & (frames[-1]["features"]["alpha"] != 0.0)).mean()))
        return 0
    features = None
    own_filter = args.guided or args.preview is not None or args.guided_budget is not None   # the call's own image is the filtered one
    if (args.denoise and not own_filter) or args.features or args.denoise_select or args.denoise_regress:
        if args.denoise and args.passes > 1:
            print("--denoise does not combine with --passes", file=sys.stderr)
            return 1
        import copy
        fp = copy.copy(p)
        fp.spp = min(p.spp, 16)
        features = render.render_features(sc, cam, fp)
        if args.features:
            def grey(a):
                return Image.fromarray(np.minimum(np.maximum(a, 0.0) * 255.0 + 0.5, 255.0).astype(np.uint8), "L")
            Image.fromarray(render.quantise_rgba8(features["albedo"]), "RGBA").save(args.features + "_albedo.png")
            rgb = np.minimum(np.maximum(features["normal"] * 0.5 + 0.5, 0.0) * 255.0 + 0.5, 255.0).astype(np.uint8)
            Image.fromarray(np.ascontiguousarray(rgb), "RGB").save(args.features + "_normal.png")
            grey(features["depth"] / max(features["depth"].max(), 1e-300)).save(args.features + "_depth.png")
            grey(features["alpha"]).save(args.features + "_alpha.png")
            print("features (%d spp, %.1f ms) written to %s_{albedo,normal,depth,alpha}.png" % (fp.spp, features["stats"].kernel_ms, args.features))

    def finish(linear, rgba, stderr):
        """The image as it is written: denoised when asked for."""
        if not args.denoise or own_filter:
            return np.ascontiguousarray(rgba)
        _, out, _, ms = render.denoise(linear, features, stderr, iterations=args.denoise_iterations, want_ms=True)
        print("denoised: %d iterations, %.2f ms" % (args.denoise_iterations, ms))
        return out

    if args.noise is not None:
        if args.pass_spp < 1:
            print("--pass-spp must be at least 1", file=sys.stderr)
            return 1
        if p.spp % args.pass_spp:   # the cap is a whole number of passes: the scene's default spp (200 for scene 7) rounds up
            cap = (p.spp + args.pass_spp - 1) // args.pass_spp * args.pass_spp
            print("cap %d spp rounded up to %d, a multiple of --pass-spp %d" % (p.spp, cap, args.pass_spp))
            p.spp = cap
        per_rank = ""
        if refine is not None and (refine[2] > w or refine[3] > h):
            print("--refine %s reaches outside the %dx%d frame" % (args.refine, w, h), file=sys.stderr)
            return 1
        rounds = ""
        state = None
        if args.resume is not None:
            state = load_state(args.resume)
            if state is None:
                return 1
        if args.guided:
            g = render.render_adaptive_denoised(sc, cam, p, args.pass_spp, args.noise, args.abs_noise, iterations=args.denoise_iterations,
                                                want_state=args.save_state is not None)
            lin, rgba, spp_map, se, st, state = g["linear"], g["rgba8"], g["spp"], g["stderr"], g["stats"], g["state"]
            rounds = "; guided: %d rounds of %d, %d denoise iterations each" % (g["rounds"], p.spp // args.pass_spp, args.denoise_iterations)
        elif args.preview is not None:
            g = render.render_preview(sc, cam, p, args.preview, args.pass_spp, args.noise, args.abs_noise, iterations=args.denoise_iterations,
                                      want_state=args.save_state is not None)
            lin, rgba, spp_map, se, st, state = g["linear"], g["rgba8"], g["spp"], g["raw_stderr"], g["stats"], g["state"]
            rounds = "; preview: 1 pixel in %d, %d of %d pixels hold a value, %d denoise iterations" % (4 ** args.preview, int(g["valid"].sum()), w * h,
                                                                                                      args.denoise_iterations)
        elif args.guided_budget is not None:
            g = render.render_adaptive_budget_denoised(sc, cam, p, args.guided_budget, state=state, pass_spp=args.pass_spp, rel_error=args.noise,
                                                       abs_error=args.abs_noise, iterations=args.denoise_iterations,
                                                       want_state=args.save_state is not None)
            lin, rgba, spp_map, se, st, state = g["linear"], g["rgba8"], g["spp"], g["stderr"], g["stats"], g["state"]
            rounds = "; guided budget: %d of %d samples in %d rounds, %d of %d pixels hold samples, %d denoise iterations each" % (
                st.samples, args.guided_budget, g["rounds"], int((spp_map > 0).sum()), w * h, args.denoise_iterations)
        elif args.budget is not None:
            lin, rgba, spp_map, se, st, state, n_rounds = render.render_adaptive_budget(sc, cam, p, args.budget, state=state, pass_spp=args.pass_spp,
                                                                                       rel_error=args.noise, abs_error=args.abs_noise,
                                                                                       want_state=args.save_state is not None)
            rounds = "; budget: %d of %d samples in %d rounds, %d of %d pixels hold samples" % (st.samples, args.budget, n_rounds,
                                                                                             int((spp_map > 0).sum()), w * h)
        elif refine is not None or args.resume is not None or args.save_state is not None:
            if refine is not None:
                lin, rgba, spp_map, se, sts, state = render.render_adaptive_region(sc, cam, p, *refine, state=state, device_ids=devices,
                                                                                   pass_spp=args.pass_spp, rel_error=args.noise, abs_error=args.abs_noise,
                                                                                   want_state=args.save_state is not None)
            else:
                lin, rgba, spp_map, se, sts, state = render.render_adaptive_resume(sc, cam, p, state, devices, args.pass_spp, args.noise, args.abs_noise,
                                                                                   want_state=args.save_state is not None)
            if devices is not None:
                st = abi.Stats(samples=sum(x.samples for x in sts), kernel_ms=node_ms(devices, sts))
                per_rank = "; per rank: %s" % " ".join(str(x.samples) for x in sts)
            else:
                st = sts
        elif devices is not None:
            lin, rgba, spp_map, se, sts = render.render_adaptive_multi(sc, cam, p, devices, args.pass_spp, args.noise, args.abs_noise)
            st = abi.Stats(samples=sum(x.samples for x in sts), kernel_ms=node_ms(devices, sts))
            per_rank = "; per rank: %s" % " ".join(str(x.samples) for x in sts)
        else:
            lin, rgba, spp_map, se, st = render.render_adaptive(sc, cam, p, args.pass_spp, args.noise, args.abs_noise)
        if args.save_state is not None:
            save_state(args.save_state, state)
        Image.fromarray(finish(lin, rgba, se), "RGBA").save(args.out)
        if args.spp_map:
            grey = np.minimum(spp_map.astype(np.float64) / p.spp * 255.0 + 0.5, 255.0).astype(np.uint8)
            Image.fromarray(grey, "L").save(args.spp_map)
        full = w * h * p.spp
        if refine is not None:
            print("window %dx%d at (%d, %d) of %dx%d" % (refine[2] - refine[0], refine[3] - refine[1], refine[0], refine[1], w, h))
        print("%.3fs (adaptive: %d samples traced of %d = %dx%dx%d, %.1f %%; kernels %.1f ms%s%s)"
              % (time.time() - t0, st.samples, full, w, h, p.spp, 100.0 * st.samples / full, st.kernel_ms, per_rank, rounds))
        return 0
    if args.passes > 1:
        def show(k, linear):
            Image.fromarray(render.quantise_rgba8(linear), "RGBA").save(args.out)
            print("pass %d/%d written" % (k + 1, args.passes))
        _, rgba, _ = render.render_host_passes(sc, cam, p, args.passes, on_pass=show)
        print("%.3fs" % (time.time() - t0))
        return 0
    if devices is not None:
        lin, rgba, sts = render.render_multi(sc, cam, p, devices)
        Image.fromarray(np.ascontiguousarray(rgba), "RGBA").save(args.out)
        ms = node_ms(devices, sts)
        print("%.3fs (%d ranks, trace kernels %.1f ms, %.1f Msamples/s)" % (time.time() - t0, len(sts), ms,
                                                                           sum(x.samples for x in sts) / max(ms, 1e-9) / 1e3))
        return 0
    if args.denoise_nlm:
        if p.spp < 2 or p.spp % 2:
            print(EVEN_SPP % ("--denoise-nlm", p.spp), file=sys.stderr)
            return 1
        (lin_a, _, st_a), (lin_b, _, st_b) = render.render_halves(sc, cam, p)
        out = render.denoise_nlm(lin_a, lin_b, search_radius=args.nlm_search_radius, patch_radius=args.nlm_patch_radius, k=args.nlm_k, want_ms=True)
        Image.fromarray(out["rgba8"], "RGBA").save(args.out)
        ms = st_a.kernel_ms + st_b.kernel_ms
        print("%.3fs (two halves of %d spp: trace kernels %.1f ms, %.1f Msamples/s; non-local means %.2f ms)"
              % (time.time() - t0, p.spp // 2, ms, (st_a.samples + st_b.samples) / max(ms, 1e-9) / 1e3, out["ms"]))
        return 0
    if args.denoise_select:
        (lin_a, _, st_a), (lin_b, _, st_b) = render.render_halves(sc, cam, p)
        out = render.denoise_select(lin_a, lin_b, features, iterations=args.denoise_iterations, search_radius=args.nlm_search_radius,
                                    patch_radius=args.nlm_patch_radius, k=args.nlm_k, margin=args.select_margin, want_ms=True)
        Image.fromarray(out["rgba8"], "RGBA").save(args.out)
        if args.blend_map:
            Image.fromarray(np.minimum(out["blend"] * 255.0 + 0.5, 255.0).astype(np.uint8), "L").save(args.blend_map)
        ms = st_a.kernel_ms + st_b.kernel_ms
        print("%.3fs (two halves of %d spp: trace kernels %.1f ms, %.1f Msamples/s; features %.1f ms; both filters and the selection %.2f ms)"
              % (time.time() - t0, p.spp // 2, ms, (st_a.samples + st_b.samples) / max(ms, 1e-9) / 1e3, features["stats"].kernel_ms, out["ms"]))
        print("selection: %.1f %% of the pixels took non-local means, %.1f %% the feature-guided filter, %.1f %% a blend of the two"
              % (100.0 * (out["blend"] == 1.0).mean(), 100.0 * (out["blend"] == 0.0).mean(),
                 100.0 * ((out["blend"] > 0.0) & (out["blend"] < 1.0)).mean()))
        return 0
    if args.denoise_regress:
        (lin_a, _, st_a), (lin_b, _, st_b) = render.render_halves(sc, cam, p)
        mask = 7 if args.regress_features is None else regress_mask(args.regress_features)
        out = render.denoise_regress(lin_a, lin_b, None, None, features, mask=mask, demodulate=not args.no_demodulate, ridge=args.ridge or 0.0,
                                     search_radius=args.nlm_search_radius, patch_radius=args.nlm_patch_radius, k=args.nlm_k, want_ms=True)
        Image.fromarray(out["rgba8"], "RGBA").save(args.out)
        if args.fit_map:
            Image.fromarray((out["fit"] * 127.5).astype(np.uint8), "L").save(args.fit_map)
        ms = st_a.kernel_ms + st_b.kernel_ms
        print("%.3fs (two halves of %d spp: trace kernels %.1f ms, %.1f Msamples/s; features %.1f ms; first-order regression %.2f ms)"
              % (time.time() - t0, p.spp // 2, ms, (st_a.samples + st_b.samples) / max(ms, 1e-9) / 1e3, features["stats"].kernel_ms, out["ms"]))
        print("regression: features %s, %s; %.1f %% of the pixels used the first-order fit in both directions, %.1f %% in neither"
              % ("".join(ch for ch, bit in (("a", 1), ("n", 2), ("z", 4)) if mask & bit) or "none", "colour" if args.no_demodulate else "colour / albedo",
                 100.0 * (out["fit"] == 2.0).mean(), 100.0 * (out["fit"] == 0.0).mean()))
        return 0
    lin, rgba, st = render.render_host(sc, cam, p)
    Image.fromarray(finish(lin, rgba, None), "RGBA").save(args.out)
    print("%.3fs (trace kernel %.1f ms, %.1f Msamples/s)" % (time.time() - t0, st.kernel_ms,
                                                          st.samples / max(st.kernel_ms, 1e-9) / 1e3))
    return 0


if __name__ == "__main__":
    sys.exit(main())
