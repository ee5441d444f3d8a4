"""TEST INFRASTRUCTURE for rttnw_budget_select and rttnw_render_adaptive_budget: a numpy restatement of the priority and of the selection, written
from the contract in include/rttnw_hip.h (not from rttnw_amd/csrc/budget_select.hpp), and the loader of the host build of that header
(tests/budget_host).  numpy's element-wise double arithmetic is IEEE and fuses nothing, so the three — device, host build, this file — must agree
bit for bit.  The colour and the error of a pixel without samples are replaced by 0 before any arithmetic here."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def priority(linear, stderr, spp, cap, rel_error, abs_error):
    """rho of every pixel, HxW f64: 0 for a non-candidate, +inf for a pixel without samples, else max over r, g, b of se / (abs + rel * value) where
    that exceeds the tolerance (and +inf where the quotient is not a finite positive number)."""
    spp = np.asarray(spp)
    held = spp > 0
    v = np.where(held[..., None], np.asarray(linear, dtype=np.float64), 0.0)
    se = np.where(held[..., None], np.asarray(stderr, dtype=np.float64), 0.0)
    with np.errstate(all="ignore"):
        t = np.float64(abs_error) + np.float64(rel_error) * v
        within = se <= t
        e = se / t
        e = np.where((e > 0.0) & np.isfinite(e), e, np.inf)
        e = np.where(within, 0.0, e)
    rho = e.max(axis=-1)
    rho = np.where(spp >= cap, 0.0, rho)
    return np.where(held, rho, np.inf)


def select(linear, stderr, spp, cap, rel_error, abs_error, max_pixels):
    """The contract of rttnw_budget_select restated: (mask HxW u8, priority HxW f64, m)."""
    rho = priority(linear, stderr, spp, cap, rel_error, abs_error)
    flat = rho.reshape(-1)
    cand = np.flatnonzero(flat > 0.0)
    order = cand[np.lexsort((cand, -flat[cand]))]          # rho descending, then row-major index ascending
    m = min(len(order), int(max_pixels))
    mask = np.zeros(flat.shape, dtype=np.uint8)
    mask[order[:m]] = 1
    return mask.reshape(rho.shape), rho, m


def host():
    """bh_select of tests/budget_host, wrapped like `select`; `.digits_roundtrip(hi, lo)` is the radix select's view of a key held to the key."""
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "budget_host"), "-s"], check=True)
    lib = C.CDLL(os.path.join(ROOT, "tests", "budget_host", "libbudget_host.so"))
    lib.bh_select.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_double, C.c_double, C.c_uint64,
                              C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    lib.bh_select.restype = C.c_int
    lib.bh_digits_roundtrip.argtypes = [C.c_uint64, C.c_uint32]
    lib.bh_digits_roundtrip.restype = C.c_int

    def run(linear, stderr, spp, cap, rel_error, abs_error, max_pixels):
        lin = np.ascontiguousarray(linear, dtype=np.float64)
        se = np.ascontiguousarray(stderr, dtype=np.float64)
        n = np.ascontiguousarray(spp, dtype=np.uint32)
        h, w = n.shape
        assert lin.shape == (h, w, 3) and se.shape == (h, w, 3)
        mask, rho, m = np.zeros((h, w), dtype=np.uint8), np.zeros((h, w)), C.c_uint64(0)
        assert lib.bh_select(w, h, lin.ctypes.data, se.ctypes.data, n.ctypes.data, cap, rel_error, abs_error, int(max_pixels), mask.ctypes.data,
                             rho.ctypes.data, C.byref(m)) == 0
        return mask, rho, int(m.value)
    run.digits_roundtrip = lambda hi, lo: lib.bh_digits_roundtrip(int(hi), int(lo))
    return run


# ---- the hostile maps of tests/test_budget_cpu.py and tests/test_gpu_budget_select.py: name -> (linear, stderr, spp, cap, rel_error, abs_error)

def _base(w, h, seed):
    rng = np.random.default_rng(seed)
    lin = rng.uniform(0.0, 2.0, (h, w, 3))
    se = lin * rng.uniform(0.0, 0.1, (h, w, 3)) + rng.uniform(0.0, 0.01, (h, w, 3))
    spp = (rng.integers(1, 8, (h, w)) * 16).astype(np.uint32)
    return rng, lin, se, spp


def hostile_maps(w, h):
    out = {}
    rng, lin, se, spp = _base(w, h, 1)
    out["mixed"] = (lin, se, spp, 128, 0.05, 0.01)                           # candidates, stopped pixels and pixels at the cap
    rng, lin, se, spp = _base(w, h, 2)
    out["all equal"] = (np.full((h, w, 3), 0.5), np.full((h, w, 3), 0.25), np.full((h, w), 16, np.uint32), 128, 0.1, 0.0)
    out["all inf"] = (lin, se, np.zeros((h, w), np.uint32), 128, 0.05, 0.01)
    out["no candidate"] = (lin, np.zeros((h, w, 3)), spp, 128, 0.05, 0.01)
    base = np.full((h, w, 3), 1.0)
    ulp = np.ones((h, w, 3))
    ulp[..., 0] = 3.0 + rng.integers(0, 3, (h, w)) * np.spacing(3.0)           # priorities that differ in the last mantissa bit only
    out["last bit"] = (base, ulp, np.full((h, w), 32, np.uint32), 128, 1.0, 0.0)
    zero = lin.copy()
    zero[rng.uniform(size=(h, w)) < 0.5] = 0.0
    out["value 0, abs 0"] = (zero, se + 1e-3, spp, 128, 0.05, 0.0)           # division by zero: +inf
    tiny = 5e-324 * rng.integers(0, 2000, (h, w, 3))                           # quotients that are whole numbers, or overflow to +inf
    tiny[rng.uniform(size=(h, w)) < 0.2] = 1.0
    out["subnormal abs"] = (np.zeros((h, w, 3)), tiny, spp, 128, 0.0, 5e-324)
    inf_se = se.copy()
    inf_se[rng.uniform(size=(h, w)) < 0.3] = np.inf                          # fewer than two chunks
    out["se inf"] = (lin, inf_se, spp, 128, 0.05, 0.01)
    capped = np.where(rng.uniform(size=(h, w)) < 0.5, 128, spp).astype(np.uint32)
    out["at the cap, huge error"] = (lin, np.where((capped == 128)[..., None], 1e30, se), capped, 128, 0.05, 0.01)
    holes = spp.copy()
    holes[rng.uniform(size=(h, w)) < 0.4] = 0
    poisoned_lin, poisoned_se = lin.copy(), se.copy()
    poisoned_lin[holes == 0] = np.nan
    poisoned_se[holes == 0] = np.nan
    out["NaN where spp is 0"] = (poisoned_lin, poisoned_se, holes, 128, 0.05, 0.01)
    return out


def budgets(rho, tie_groups=None):
    """The values of m a map is held to: 0, 1, candidates - 1, candidates, candidates + 5 and a value inside EVERY tie group — or, with
    `tie_groups` = n, inside the n groups of highest and the n of lowest priority only (the device tests on large frames, which say so)."""
    flat = rho.reshape(-1)
    cand = np.sort(flat[flat > 0.0])[::-1]
    n = len(cand)
    ms = {0, 1, max(n - 1, 0), n, n + 5}
    values, first, counts = np.unique(-cand, return_index=True, return_counts=True)
    ties = [(int(f), int(c)) for f, c in zip(first, counts) if c > 1]
    for f, c in (ties if tie_groups is None else ties[:tie_groups] + ties[-tie_groups:]):
        ms.add(f + c // 2)                                                    # cuts the group: f .. f + c - 1 are its places
    return sorted(ms)
