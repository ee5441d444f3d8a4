"""Host lockstep model of the lane-owns-path kernel (tests/run_ahead_host hostsim_wave_model_ahead: tests/hostsim's policy 4) with RUN-AHEAD in its trips, priced in instructions.

    python profiles/experiments/wave_run_ahead.py [scene [waves [jobs per wave]]]

Per trip length (2, 3, 4 node steps) and form (0 the trip without run-ahead, 1 stash points before every node step / the first / the first two, 2 the
leaf put aside inside the node step's descend): step executions and the lanes they serve, records put aside, and the walk's vector instructions per sample from the STATIC counts of
the compiled regions (KERNELS.md: the trip's body is 716 instructions = two node steps of NODE and a leaf step of LEAF; a stash point is its test,
TEST instructions wherever a walking lane passes it, and its pop, POP instructions where a lane puts a record aside; form 2 adds SEL instructions of
selects to every node step instead and saves the pop).  The model counts executions, not lanes: an instruction costs the same for 1 lane or 64."""
import ctypes as C, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from rttnw_amd import abi, scene as S
lib = C.CDLL(os.path.join(ROOT, "tests", "run_ahead_host", "librun_ahead_host.so"))
b = abi.Binding(lib, "rttnw_", abi.BUILDER_FUNCS); b.add([("builder", C.c_void_p, [])])
scenes = abi.Binding(C.CDLL(os.path.join(ROOT, "rttnw_amd", "host", "librttnw_scenes.so")), "", abi.SCENES_FUNCS)
lib.hostsim_wave_model_ahead.argtypes = [C.c_void_p, C.POINTER(abi.CameraDesc), C.POINTER(abi.Params), C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p]
name = sys.argv[1] if len(sys.argv) > 1 else "final_scene"
waves = int(sys.argv[2]) if len(sys.argv) > 2 else 24
jobs = int(sys.argv[3]) if len(sys.argv) > 3 else 512
earth = S.load_earth() if name in ("final_scene", "earth") else None
sc, setup = S.build(b, scenes, name, earth)
cam, p = S.params_for(setup, 800, 800, 1000)
p.precision = abi.F64
# static instruction counts, final_scene f64 (the headline instantiation): the node step's ~110, the leaf step the rest of the trip's 716.  The
# compiled kernel with run-ahead is 109 instructions longer at two node steps per trip and 148 at three (6235 against 6126, 6501 against 6353:
# a gfx950 cross-compile of render_f64.hip): ~50 a stash point — its test and branch ~15, the pop behind it (LDS entry or spill strip) ~35 —
# and ~9 of selects in the leaf step.  Form 2 was not compiled: its selects are an estimate.
NODE, LEAF, TEST, POP, LEAF_SEL, SEL = 110, 496, 15, 35, 9, 8
T = 56   # lanes waiting that start a shade phase: 64 - RT_ASYNC_SLACK
def run(steps, form, mask=15):
    out = np.zeros(64, dtype=np.uint64)
    assert lib.hostsim_wave_model_ahead(sc.handle, C.byref(cam), C.byref(p), steps, form, mask, T, waves, jobs, out.ctypes.data) == 0
    return [int(x) for x in out]
base = None
print("%s 800x800 spp 1000 f64, %d waves x %d jobs, shade phase at %d waiting lanes; per sample" % (name, waves, jobs, T))
print("trip        | node exec (lanes) | leaf exec (lanes) | node / leaf lane-steps | put aside [by stash point] | walk cost (N=1, L=2.46) | walk instructions")
for form, mask in ((0, 15), (1, 15), (1, 1), (1, 3), (2, 15)):   # (mask: the stash points kept, bit k = before node step k; 1 is the kernel's)
    for steps in (2, 3, 4):
        o = run(steps, form, mask)
        nexec, nlanes, lexec, llanes, samples = o[1], o[2], o[3], o[4], max(1, o[5])
        assert o[38] == 0, "a lane kept a record put aside beyond its trip"
        units = (nexec + 2.46 * lexec) / samples
        instr = NODE * nexec + LEAF * lexec
        if form == 1:
            instr += TEST * o[39] + POP * o[37] + LEAF_SEL * lexec
        elif form == 2:
            instr += SEL * nexec + LEAF_SEL * lexec
        instr /= samples
        if base is None:
            base = (units, instr)
        print("%s %dN+L | %.3f (%.1f) | %.3f (%.1f) | %.2f / %.2f | %.2f [%s] | %.3f (%+.1f %%) | %.0f (%+.1f %%)" % (
            ("today        ", "stash pt %-4s" % {15: "all", 1: "1st", 3: "1+2"}[mask], "descend      ")[form], steps, nexec / samples, nlanes / max(1, nexec), lexec / samples, llanes / max(1, lexec),
            nlanes / samples, llanes / samples, o[36] / samples, " ".join("%.2f" % (o[60 + k] / samples) for k in range(steps)) if form == 1 else "", units, 100 * (units / base[0] - 1), instr, 100 * (instr / base[1] - 1)))
