"""tests/abi_cases.py bites: declared_alike refuses a header prototype with two arguments swapped, an ffi.rs argument of the wrong mutability and a
ctypes table with one argtype changed, and break_state changes exactly the double it addresses.  In-memory strings only: no library call, no process."""
import ctypes as C

import numpy as np
import pytest

import abi_cases
from abi_cases import STATE_HEADER_DOUBLES, STATE_RECORD_DOUBLES

ARGS = [("width", "uint32_t", "u32", C.c_uint32), ("state_in", "const double*", "*const f64", C.c_void_p),
        ("state_out", "double*", "*mut f64", C.c_void_p), ("stats", "rttnw_stats*", "*mut rttnw_stats", C.c_void_p)]
HEADER = "int rttnw_probe(uint32_t width, const double* state_in,\n              double *state_out, rttnw_stats* stats);\n"
FFI = "extern \"C\" {\n    pub fn rttnw_probe(width: u32, state_in: *const f64, state_out: *mut f64, stats: *mut rttnw_stats) -> c_int;\n}\n"
FUNCS = [("probe", C.c_int, [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p])]


def _alike(header=HEADER, ffi=FFI, funcs=FUNCS, **kw):
    abi_cases.declared_alike("probe", ARGS, header=header, ffi=ffi, funcs=funcs, **kw)


def test_declared_alike_accepts_what_agrees():
    _alike()


@pytest.mark.parametrize("what,broken,where", [
    ("two header arguments swapped", dict(header=HEADER.replace("const double* state_in,\n              double *state_out", "double *state_out, const double* state_in")),
     "include/rttnw_hip.h"),
    ("a header type", dict(header=HEADER.replace("uint32_t width", "uint64_t width")), "include/rttnw_hip.h"),
    ("the header's return type", dict(header=HEADER.replace("int rttnw_probe", "void rttnw_probe")), "include/rttnw_hip.h"),
    ("ffi.rs mutability", dict(ffi=FFI.replace("state_out: *mut f64", "state_out: *const f64")), "ffi.rs"),
    ("ffi.rs argument name", dict(ffi=FFI.replace("state_in:", "state:")), "ffi.rs"),
    ("ffi.rs return type", dict(ffi=FFI.replace("c_int", "u64")), "ffi.rs"),
    ("one argtype", dict(funcs=[("probe", C.c_int, [C.c_uint32, C.c_void_p, C.POINTER(C.c_double), C.c_void_p])]), "PRODUCT_FUNCS"),
    ("an argtype dropped", dict(funcs=[("probe", C.c_int, [C.c_uint32, C.c_void_p, C.c_void_p])]), "PRODUCT_FUNCS"),
    ("the restype", dict(funcs=[("probe", C.c_uint64, FUNCS[0][2])]), "PRODUCT_FUNCS"),
])
def test_declared_alike_refuses(what, broken, where):
    with pytest.raises(AssertionError) as e:
        _alike(**broken)
    assert "rttnw_probe" in str(e.value) and where in str(e.value), what


def test_break_state_changes_exactly_the_addressed_double():
    p, a, cam = abi_cases.params(spp_chunk=4), abi_cases.adaptive(), abi_cases.camera()
    st = abi_cases.hand_made_state(p, a, cam)
    assert st.shape == (STATE_HEADER_DOUBLES + STATE_RECORD_DOUBLES * 16 * 16,)
    for what, at in ((4, 4), (30, 30), (("k", 15.0), STATE_HEADER_DOUBLES + 5 * STATE_RECORD_DOUBLES + 7),
                     (("n", float("nan")), STATE_HEADER_DOUBLES + 5 * STATE_RECORD_DOUBLES + 3)):
        broken = abi_cases.break_state(st, what)
        assert np.flatnonzero(broken.view(np.uint64) != st.view(np.uint64)).tolist() == [at], what
    nan_header = st.copy()
    nan_header[12] = np.nan                          # a NaN word cannot be broken by adding to it: it becomes 0
    assert abi_cases.break_state(nan_header, 12)[12] == 0.0
