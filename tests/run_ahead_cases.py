"""The scenes the run-ahead tests render (tests/test_run_ahead_cpu.py on the host build, tests/test_gpu_run_ahead.py on the device), through any
binding.  Each case: (Scene, CameraDesc, Params factory) at the size the issue of the change set; none of them has a walk that changes frames.

  final_scene      48x48 spp 4: every record kind, stack_depth 24 — beyond the 16 stack entries a lane keeps in LDS
  hostile-*        the three worlds of tests/hostile_world.py at their own 33x33 spp 3 (first camera)
  ties             pairs of coincident spheres and coincident cubes with different solid colours, both list orders: t == closest, prim_seq decides
  one / two        one sphere; two spheres: a pop finds the stack empty while a record is put aside"""
import ctypes as C
import os
import subprocess

import hostile_world
from rttnw_amd import abi
from rttnw_amd import scene as S

NAMES = ["final_scene", "hostile-origin", "hostile-milli", "hostile-1e6", "ties", "one", "two"]


_HOST = []


def host_binding():
    """The host build of the tracing core with the run-ahead drivers (tests/run_ahead_host: tests/hostsim's code and exports, plus
    hostsim_render_run_ahead, hostsim_wave_model_ahead and hostsim_plan_run_ahead), built on first use — a binding scenes can be built through."""
    if not _HOST:
        here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "run_ahead_host")
        subprocess.run(["make", "-C", here, "-s"], check=True)
        lib = C.CDLL(os.path.join(here, "librun_ahead_host.so"))
        b = abi.Binding(lib, "rttnw_", abi.BUILDER_FUNCS)
        b.add([("builder", C.c_void_p, [])])
        lib.hostsim_render.restype = C.c_int
        lib.hostsim_render.argtypes = [C.c_void_p, C.POINTER(abi.CameraDesc), C.POINTER(abi.Params), C.c_void_p, C.POINTER(abi.Stats), C.c_int]
        lib.hostsim_render_run_ahead.restype = C.c_int
        lib.hostsim_render_run_ahead.argtypes = [C.c_void_p, C.POINTER(abi.CameraDesc), C.POINTER(abi.Params), C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        lib.hostsim_plan_run_ahead.restype = C.c_int
        lib.hostsim_plan_run_ahead.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int]
        lib.hostsim_scene_dims.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        _HOST.append(b)
    return _HOST[0]


def _ties(binding):
    sc = S.Scene(binding, 5)
    red, green, blue, yellow = (sc.lambertian(c) for c in ((0.9, 0.1, 0.1), (0.1, 0.9, 0.1), (0.1, 0.1, 0.9), (0.9, 0.9, 0.1)))
    items = []
    for k, (x, first, second) in enumerate(((-3.0, red, green), (-1.0, green, red))):       # the same pair of spheres in both list orders
        items += [sc.sphere((x, 0.0, 0.0), 0.8, first), sc.sphere((x, 0.0, 0.0), 0.8, second)]
    for k, (x, first, second) in enumerate(((1.0, blue, yellow), (3.0, yellow, blue))):     # ... and of cubes
        items += [sc.cube((x - 0.7, -0.7, -0.7), (x + 0.7, 0.7, 0.7), first), sc.cube((x - 0.7, -0.7, -0.7), (x + 0.7, 0.7, 0.7), second)]
    items.append(sc.sphere((0.0, -100.8, 0.0), 100.0, sc.lambertian((0.5, 0.5, 0.5))))
    sc.set_world(sc.list([sc.bvh_tree(sc.list(items))]))
    sc.commit()
    return sc, S.camera_desc((0.0, 1.5, -9.0), (0.0, 0.0, 0.0), 50.0, 1.0), dict(width=16, height=16, spp=4, background=(0.7, 0.8, 1.0), seed=3)


def _spheres(binding, n):
    sc = S.Scene(binding, 6)
    grey = sc.lambertian((0.6, 0.6, 0.6))
    items = [sc.sphere((0.0, 0.0, 0.0), 1.0, grey)] + ([sc.sphere((1.5, 0.0, 0.5), 0.7, sc.metal((0.8, 0.8, 0.8), 0.0))] if n == 2 else [])
    sc.set_world(sc.list([sc.bvh_tree(sc.list(items))]))
    sc.commit()
    return sc, S.camera_desc((0.0, 0.5, -5.0), (0.5, 0.0, 0.0), 45.0, 1.0), dict(width=8, height=8, spp=2, background=(0.7, 0.8, 1.0), seed=2)


def case(binding, scenes_lib, earth, name):
    """(Scene, CameraDesc, make) with make(precision, **kw) -> Params."""
    if name == "final_scene":
        sc, setup = S.build(binding, scenes_lib, name, earth)

        def make(precision, **kw):
            return S.params_for(setup, 48, 48, 4, precision=precision, **kw)[1]
        return sc, S.params_for(setup, 48, 48, 4)[0], make
    if name.startswith("hostile-"):
        scale, shift = hostile_world.WORLDS[hostile_world.WORLD_IDS.index(name[len("hostile-"):])]
        sc, _ = hostile_world.scene(binding, scale, shift)
        return sc, hostile_world.cameras(scale, shift)[0], lambda precision, **kw: hostile_world.params(precision, scale, **kw)
    sc, cam, base = _ties(binding) if name == "ties" else _spheres(binding, 1 if name == "one" else 2)
    return sc, cam, lambda precision, **kw: S.make_params(base["width"], base["height"], base["spp"], background=base["background"], seed=base["seed"],
                                                          precision=precision, **kw)
