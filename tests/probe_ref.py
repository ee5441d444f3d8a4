"""TEST INFRASTRUCTURE for rttnw_temporal_probe: a numpy restatement of the contract in include/rttnw_hip.h (not of rttnw_amd/csrc/probe.hpp),
and the loader of the host build of that header (tests/probe_host).  The contract's geometry and acceptance are rttnw_temporal_accumulate's, so the
restatement takes them from that call's restatement (temporal_ref.where_it_was, temporal_ref.tap_acceptance) and restates what the probe does with
them: the length without the colour, and the multiplier.  numpy's element-wise double arithmetic is IEEE and fuses nothing, and every sum below
adds its terms one at a time in the header's order, so the three — device, host build, this file — must agree bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np

import temporal_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = {"boost": 8, "fill": 8.0}
OUTPUTS = ("length", "prev_xy", "multiplier")
_LIB = []


def _lib():
    if not _LIB:
        subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "probe_host"), "-s"], check=True)
        lib = C.CDLL(os.path.join(ROOT, "tests", "probe_host", "libprobe_host.so"))
        lib.ph_temporal_probe.argtypes = [C.c_uint32, C.c_uint32] + [C.c_void_p] * 9 + [C.c_uint32, C.c_double, C.c_double, C.c_uint32, C.c_double] + [C.c_void_p] * 3
        lib.ph_temporal_probe.restype = C.c_int
        _LIB.append(lib)
    return _LIB[0]


def _arrays(features, history):
    f = [np.ascontiguousarray(features[k], dtype=np.float64) for k in ("normal", "depth", "alpha")]
    prev = [None] * 4
    if history is not None:
        pf = history["features"]
        prev = [np.ascontiguousarray(a, dtype=np.float64) for a in (history["length"], pf["normal"], pf["depth"], pf["alpha"])]
    return f, prev


def host():
    """ph_temporal_probe of tests/probe_host, wrapped: the arguments of `probe` below -> dict of OUTPUTS."""
    lib = _lib()

    def run(features, cam, history=None, boost=0, fill=0.0, max_history=0, depth_tolerance=0.0, normal_min=0.0):
        f, prev = _arrays(features, history)
        h, w = f[1].shape
        out = {"length": np.zeros((h, w)), "prev_xy": np.zeros((h, w, 2)), "multiplier": np.zeros((h, w), dtype=np.uint8)}
        ptr = lambda a: None if a is None else a.ctypes.data
        rc = lib.ph_temporal_probe(w, h, C.addressof(cam), None if history is None else C.addressof(history["cam"]), *[ptr(a) for a in f],
                                   *[ptr(a) for a in prev], max_history, depth_tolerance, normal_min, boost, fill, *[ptr(out[name]) for name in OUTPUTS])
        assert rc == 0
        return out
    return run


def multiplier(length, hit, boost=0, fill=0.0):
    """The contract's multiplier rule: k = floor(fill / (Lp + 1)); the largest of 1, 2, 4, 8 that is <= min(k, boost); 1 where k < 1 (or NaN) and
    on a miss."""
    boost, fill = boost or DEFAULTS["boost"], fill or DEFAULTS["fill"]
    with np.errstate(all="ignore"):
        k = np.floor(fill / (length + 1.0))
    m = np.ones(np.shape(length), dtype=np.uint8)
    for level in (2, 4, 8):
        if level <= boost:
            m = np.where(k >= float(level), np.uint8(level), m)
    return np.where(hit, m, np.uint8(1)).astype(np.uint8)


def probe(features, cam, history=None, boost=0, fill=0.0, max_history=0, depth_tolerance=0.0, normal_min=0.0):
    """The contract of rttnw_temporal_probe restated: dict of OUTPUTS."""
    (normal, depth, alpha), prev = _arrays(features, history)
    h, w = depth.shape
    length, xy = np.zeros((h, w)), np.full((h, w, 2), np.nan)
    if history is not None:
        fx, fy, zq, ok = temporal_ref.where_it_was(w, h, cam, history["cam"], depth, alpha)
        xy[ok] = np.stack([fx, fy], axis=-1)[ok]
        sw, sl = np.zeros((h, w)), np.zeros((h, w))
        with np.errstate(all="ignore"):
            for acc, wt, at in temporal_ref.tap_acceptance(fx, fy, zq, ok, normal, [None, None] + prev, depth_tolerance, normal_min):
                sw = np.where(acc, sw + wt, sw)
                sl = np.where(acc, sl + wt * prev[0][at], sl)
            found = ok & (sw > 0.0)
            length[found] = (sl / sw)[found]
    return {"length": length, "prev_xy": xy, "multiplier": multiplier(length, alpha != 0.0, boost, fill)}


def grown(length, max_history=0):
    """What rttnw_temporal_accumulate's out_length is, from the probe's: Lp == 0 ? 1 : min(Lp + 1, max_history), min as that contract takes it."""
    most = float(max_history or temporal_ref.DEFAULTS["max_history"])
    with np.errstate(all="ignore"):
        g = length + 1.0
    return np.where(length == 0.0, 1.0, np.where(g < most, g, most))
