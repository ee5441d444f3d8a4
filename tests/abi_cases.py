"""What the no-GPU tests of the C ABI's entry points share (tests/test_*_abi_cpu.py, tests/test_adaptive_cpu.py, tests/test_adaptive_state_cpu.py):
the header and the Rust declarations as text, the comparison of an entry point's declaration across header, ctypes binding and Rust binding, the
arguments of a small adaptive call, the adaptive state made by hand from the layout include/rttnw_hip.h documents, the two-sided refusal check and
the command line's refusal runner.  The tables of what is refused, and every test, stay in the test files."""
import ctypes as C
import os
import re
import struct
import subprocess
import sys

import numpy as np

from rttnw_amd import abi, library
from rttnw_amd import scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def strip_c_comments(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


HEADER_TEXT = open(os.path.join(ROOT, "include", "rttnw_hip.h")).read()
HEADER = strip_c_comments(HEADER_TEXT)
FFI = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read())
RUST_SCENE = open(os.path.join(ROOT, "bindings", "rust", "src", "scene.rs")).read()
INVALID, STATE, UNSUPPORTED = -1, -2, -3
MAGIC, VERSION = 1381256791, 1
STATE_HEADER_DOUBLES, STATE_RECORD_DOUBLES = 64, 12


def declared_alike(name, args, c_ret="int", rs_ret="c_int", ct_ret=C.c_int, header=HEADER, ffi=FFI, funcs=abi.PRODUCT_FUNCS):
    """rttnw_<name> takes `args` — (name, C type, Rust type, ctypes type) each — and returns c_ret / rs_ret / ct_ret in the header's prototype, in
    ffi.rs and in the ctypes table: the same names, in the same order, with the same types."""
    m = re.search(r"\b%s rttnw_%s\((.*?)\);" % (c_ret, name), header, flags=re.S)
    assert m, "include/rttnw_hip.h does not declare %s rttnw_%s" % (c_ret, name)
    c_args = []
    for a in " ".join(m.group(1).split()).split(","):
        ctype, arg = re.match(r"(.+?)\s*(\w+)$", a.strip()).groups()
        c_args.append((arg, ctype.replace(" *", "*")))
    assert c_args == [(n, c) for n, c, _, _ in args], "rttnw_%s in include/rttnw_hip.h: %s" % (name, c_args)
    m = re.search(r"pub fn rttnw_%s\((.*?)\)\s*->\s*%s;" % (name, rs_ret), ffi, flags=re.S)
    assert m, "bindings/rust/src/ffi.rs does not declare rttnw_%s -> %s" % (name, rs_ret)
    rs_args = [tuple(x.strip() for x in a.split(":", 1)) for a in m.group(1).split(",") if ":" in a]
    assert rs_args == [(n, r) for n, _, r, _ in args], "rttnw_%s in bindings/rust/src/ffi.rs: %s" % (name, rs_args)
    proto = {n: (res, a) for n, res, a in funcs}[name]
    assert proto[0] is ct_ret and list(proto[1]) == [t for _, _, _, t in args], "rttnw_%s in abi.PRODUCT_FUNCS: %s" % (name, proto)


def exported(name):
    """The library exports rttnw_<name>, the binding lists it, and the ABI version did not move: the symbol is how a caller finds the feature."""
    lib = C.CDLL(library.HIP_LIB)
    assert hasattr(lib, "rttnw_" + name) and "rttnw_" + name in abi.exported_symbols(), name
    assert re.search(r"#define RTTNW_ABI_VERSION 3\b", HEADER)
    assert lib.rttnw_abi_version() == 3 and abi.ABI_VERSION == 3


CAM = dict(lookfrom=(0, 0, 5), lookat=(0, 0, 0), vfov=40.0, aspect=1.0)


def camera():
    return S.camera_desc(**CAM)


def params(**kw):
    """A 16x16 frame with a cap of 128 samples, and `kw` laid over it."""
    p = S.make_params(kw.pop("width", 16), kw.pop("height", 16), kw.pop("spp", 128))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def adaptive(**kw):
    a = abi.Adaptive(pass_spp=64, reserved0=0, rel_error=0.05, abs_error=0.0)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def chunks_of_a_pass(B, spp_chunk):
    """The chunks of a pass of B samples, by the rule in the header's comment at the record's k."""
    if spp_chunk:
        return -(-B // spp_chunk)
    tail = B if B < 32 else B // 32
    main = (B - tail) // 4
    return main + (B - 4 * main)


def hand_made_state(p, a, cam, n=None, k=None):
    """A valid state made by hand, from the layout the header documents: the header from the call's own arguments, every record n = B and k = the
    chunks of one pass unless given — n = k = 0 makes every record empty."""
    st = np.zeros(STATE_HEADER_DOUBLES + STATE_RECORD_DOUBLES * p.width * p.height)
    st[0:12] = [MAGIC, VERSION, p.width, p.height, a.pass_spp, p.spp_chunk, p.sample_begin, p.precision, p.max_depth, p.quirks,
                p.seed & 0xFFFFFFFF, p.seed >> 32]
    st[12] = p.t_min
    st[13:16] = list(p.background)
    st[16:31] = struct.unpack("15d", bytes(cam))
    rec = st[STATE_HEADER_DOUBLES:].reshape(-1, STATE_RECORD_DOUBLES)
    rec[:, 3] = a.pass_spp if n is None else n
    rec[:, 7] = chunks_of_a_pass(a.pass_spp, p.spp_chunk) if k is None else k
    return st


RECORD_FIELDS = {"sum": 0, "n": 3, "mu": 5, "k": 7, "m2": 10, "pad": 11}
BROKEN_PIXEL = 5


def break_state(st, what):
    """A copy of `st` with one double changed: the header word `what` (an index: + 1, a NaN becomes 0), or (record field, value) in pixel 5."""
    st = st.copy()
    if isinstance(what, int):
        st[what] = st[what] + 1.0 if st[what] == st[what] else 0.0
    else:
        field, value = what
        st[STATE_HEADER_DOUBLES:].reshape(-1, STATE_RECORD_DOUBLES)[BROKEN_PIXEL, RECORD_FIELDS[field]] = value
    return st


def refused(b, call, code, msg, name):
    """`call(scene=True)` runs on a scene that was never committed, `call(scene=False)` on none: both return `code` with a message that holds
    `msg` (and, on the scene, the entry point's `name`) — the refusal came before any device.  A `code` of None is a refusal that stands behind
    validate(), which looks at the scene before the sizes: "not committed" on a scene, "NULL" without one."""
    if code is None:
        assert call(scene=True) == STATE and "not committed" in b.last_error().decode(), msg
        assert call(scene=False) == INVALID and "NULL" in b.last_error().decode(), msg
        return
    assert call(scene=True) == code, msg
    err = b.last_error().decode()
    assert err and msg in err and name in err, (msg, err)
    assert call(scene=False) == code, msg
    assert msg in b.last_error().decode(), msg


def cli_refuses(argv, msg, tmp_path, must_not_exist=()):
    """`python -m rttnw_amd argv` in a fresh process, run in tmp_path: exit status 1, `msg` on stderr, no scene announced, and neither the image nor
    any file of `must_not_exist` (names in tmp_path) written."""
    out = tmp_path / "image.png"
    r = subprocess.run([sys.executable, "-m", "rttnw_amd"] + argv + ["--out", str(out)], cwd=tmp_path, capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert msg in r.stderr, r.stderr
    assert "Scene number" not in r.stdout and not out.exists()
    for name in must_not_exist:
        assert not (tmp_path / name).exists(), name
