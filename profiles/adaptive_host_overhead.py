"""Host overhead of seven adaptive entry points (adaptive, multi, resume, region, denoised, preview, budget), two builds of librttnw_hip.so side by side.

  python profiles/adaptive_host_overhead.py --parent /path/to/parent/librttnw_hip.so [--new PATH] [--rounds 6] [--reps 2] [--out result.json]

cornell_box 512x512, cap 64, pass_spp 16, f64, rel_error 0.05, abs_error 0.01.  The two builds run ALTERNATELY, `--rounds` times each (who goes first alternates as well), every time
in a fresh child process (RTTNW_HIP_LIB names the build) that calls each entry point once to warm up and then `--reps` times under the clock:
wall time around the Python wrapper's call, and the call's own stats.kernel_ms beside it.  What differs between two builds of the same kernels
is the host's share: wall - kernel.  Prints median / min / max per entry point and build, and whether the new build's median stays at or
below the largest value the parent showed.  A child that fails ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = H = 512
CAP, B, REL, ABS = 64, 16, 0.05, 0.01
CALLS = ("adaptive", "multi", "resume", "region", "denoised", "preview", "budget")


def measure(reps):
    sys.path.insert(0, ROOT)
    from rttnw_amd import abi, library, render
    from rttnw_amd import scene as S
    gpu = library.product()
    sc, setup = S.build(gpu, library.scenes(), "cornell_box")
    cam, p = S.params_for(setup, W, H, CAP, precision=abi.F64)
    tol = dict(pass_spp=B, rel_error=REL, abs_error=ABS)
    ms = lambda st: float(sum(s.kernel_ms for s in st)) if isinstance(st, list) else float(st.kernel_ms)
    calls = {
        "adaptive": lambda: ms(render.render_adaptive(sc, cam, p, **tol)[4]),
        "multi": lambda: ms(render.render_adaptive_multi(sc, cam, p, [0], **tol)[4]),
        "resume": lambda: ms(render.render_adaptive_resume(sc, cam, p, None, None, **tol)[4]),
        "region": lambda: ms(render.render_adaptive_region(sc, cam, p, 0, 0, W, H, **tol)[4]),
        "denoised": lambda: ms(render.render_adaptive_denoised(sc, cam, p, **tol)["stats"]),
        "preview": lambda: ms(render.render_preview(sc, cam, p, 2, **tol)["stats"]),
        "budget": lambda: ms(render.render_adaptive_budget(sc, cam, p, W * H * CAP // 2, 0, **tol)[4]),
    }
    out = {}
    for name in CALLS:
        calls[name]()                                  # warm-up: scene upload, workspaces, code objects
        out[name] = []
        for _ in range(reps):
            t0 = time.perf_counter()
            kernel_ms = calls[name]()
            out[name].append(((time.perf_counter() - t0) * 1e3, kernel_ms))
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="the parent commit's librttnw_hip.so")
    ap.add_argument("--new", default=os.path.join(ROOT, "rttnw_amd", "csrc", "librttnw_hip.so"))
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out")
    ap.add_argument("--measure", action="store_true", help="(child) measure the build RTTNW_HIP_LIB names")
    a = ap.parse_args()
    if a.measure:
        return measure(a.reps)
    if not a.parent:
        ap.error("--parent is required")
    builds = {"parent": os.path.abspath(a.parent), "new": os.path.abspath(a.new)}
    runs = {b: {c: [] for c in CALLS} for b in builds}
    for rnd in range(a.rounds):
        for b, lib in (list(builds.items()) if rnd % 2 == 0 else list(builds.items())[::-1]):  # who goes first alternates too
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--measure", "--reps", str(a.reps)], env=dict(os.environ, RTTNW_HIP_LIB=lib),
                               capture_output=True, text=True, timeout=300)
            line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                print("round %d, %s build: child ended with %d\n%s\n%s" % (rnd, b, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
                return 2
            for c, v in json.loads(line[0][7:]).items():
                runs[b][c] += v
    summary, ok = {}, True
    print("%-9s %-7s %27s %27s %27s" % ("call", "build", "wall ms  median/min/max", "kernel ms median/min/max", "host ms  median/min/max"))
    for c in CALLS:
        summary[c] = {}
        for b in builds:
            wall = [x[0] for x in runs[b][c]]
            kern = [x[1] for x in runs[b][c]]
            host = [x[0] - x[1] for x in runs[b][c]]
            summary[c][b] = {k: dict(median=statistics.median(v), min=min(v), max=max(v), n=len(v)) for k, v in (("wall", wall), ("kernel", kern), ("host", host))}
            print("%-9s %-7s " % (c, b) + " ".join("%9.3f/%8.3f/%8.3f" % (s["median"], s["min"], s["max"]) for s in summary[c][b].values()))
        within = summary[c]["new"]["wall"]["median"] <= summary[c]["parent"]["wall"]["max"]
        summary[c]["new_median_within_parent_max"] = within
        ok = ok and within
    print("new median <= parent max for every entry point: %s" % ok)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(frame=[W, H], cap=CAP, pass_spp=B, rounds=a.rounds, reps=a.reps, summary=summary, runs=runs), f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
