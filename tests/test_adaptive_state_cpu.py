"""The host side of an adaptive render's state without a GPU: the host build of rttnw_amd/csrc/adaptive_state.hpp (tests/state_host) — the one
permutation between a state's row-major records and the ranks' packed order that every adaptive entry point goes through, the state's header and
its checks — held to rttnw_amd/tiles.py, to the layout include/rttnw_hip.h documents and to what the library's exported entry points answer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import abi_cases
from rttnw_amd import abi, library, tiles
from rttnw_amd import scene as S
from test_adaptive_resume_abi_cpu import STATE_BREAKS, _call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = [(8, 8), (45, 37), (96, 96)]      # one tile; edge tiles on both axes and 6 tile columns, so the permutation wraps; whole tiles
WORLDS = [1, 2, 3, 5]                      # 5 leaves ranks with unequal tile counts
HEADER, RECORD = abi_cases.STATE_HEADER_DOUBLES, abi_cases.STATE_RECORD_DOUBLES


@pytest.fixture(scope="module")
def host():
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "state_host"), "-s"], check=True)
    lib = C.CDLL(os.path.join(ROOT, "tests", "state_host", "libstate_host.so"))
    lib.sh_place.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.sh_place.restype = C.c_uint32
    lib.sh_round_trip.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sh_round_trip.restype = None
    lib.sh_header.argtypes = [C.POINTER(abi.Params), C.POINTER(abi.Adaptive), C.POINTER(abi.CameraDesc), C.c_void_p]
    lib.sh_header.restype = None
    lib.sh_state_doubles.argtypes = [C.c_uint32, C.c_uint32]
    lib.sh_state_doubles.restype = C.c_uint64
    lib.sh_refuse.argtypes = [C.c_char_p, C.c_int, C.POINTER(abi.Params), C.POINTER(abi.Adaptive), C.POINTER(abi.CameraDesc), C.c_void_p,
                              C.POINTER(C.c_uint32), C.c_char_p, C.c_uint32]
    lib.sh_refuse.restype = C.c_int
    return lib


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("w,h", FRAMES)
def test_layout_is_the_closed_form(host, w, h, world):
    owner = np.zeros((h, w), np.uint32)
    idx = np.zeros((h, w), np.uint64)
    ppr = host.sh_place(w, h, world, owner.ctypes.data, idx.ctypes.data)
    want_owner, want_idx = tiles.packed_index(w, h, world)
    assert ppr == tiles.layout(w, h, world)["pixels_per_rank"]
    assert (owner == want_owner).all() and (idx == want_idx).all()
    assert idx.max() < ppr and owner.max() < world


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("w,h", FRAMES)
def test_scatter_then_gather_returns_the_records_bit_for_bit(host, w, h, world):
    rng = np.random.default_rng(w * 100 + world)
    ppr = tiles.layout(w, h, world)["pixels_per_rank"]
    state = np.zeros(HEADER + RECORD * w * h)
    rec = state[HEADER:].reshape(h, w, RECORD)
    rec[:] = rng.standard_normal(rec.shape)
    rec.reshape(-1)[::7] = [np.nan, -0.0, np.inf, 5e-324][world % 4]          # bit patterns a careless copy would lose; never +0.0
    assert (rec.view(np.uint64) != 0).all()
    packed = np.full((world, ppr, RECORD), 7.0)
    out = np.full_like(state, -1.0)
    host.sh_round_trip(w, h, world, state.ctypes.data, packed.ctypes.data, out.ctypes.data)
    assert (out[HEADER:].view(np.uint64) == state[HEADER:].view(np.uint64)).all()
    assert (out[:HEADER] == -1.0).all()                                        # the header is state_header's, not the permutation's
    owner, idx = tiles.packed_index(w, h, world)
    assert (packed[owner, idx].view(np.uint64) == rec.view(np.uint64)).all()
    mapped = np.zeros((world, ppr), bool)
    mapped[owner, idx] = True
    assert mapped.sum() == w * h                                               # no two pixels share a slot
    assert (packed[~mapped].view(np.uint64) == 0).all()                        # edge-tile padding and pad tiles: zero records
    assert (~mapped).sum() == world * ppr - w * h


def test_no_state_is_zero_records_everywhere(host):
    w, h, world = 45, 37, 3
    ppr = tiles.layout(w, h, world)["pixels_per_rank"]
    packed = np.full((world, ppr, RECORD), 7.0)
    out = np.full(HEADER + RECORD * w * h, -1.0)
    host.sh_round_trip(w, h, world, None, packed.ctypes.data, out.ctypes.data)
    assert (packed.view(np.uint64) == 0).all() and (out[HEADER:].view(np.uint64) == 0).all()


def test_state_header_is_the_documented_layout(host):
    cam = S.camera_desc(lookfrom=(1.5, -2, 5), lookat=(0, 0.25, 0), vfov=37.0, aspect=45 / 37, aperture=0.1, focus=4.5)
    p = abi_cases.params(width=45, height=37, spp=96, spp_chunk=4, sample_begin=32, max_depth=17, quirks=1, seed=(0xDEADBEEF << 32) | 0x80000001,
                           t_min=1e-3, precision=abi.F32)
    p.background[0], p.background[1], p.background[2] = 0.25, -0.0, 3.0
    a = abi_cases.adaptive(pass_spp=32)
    got = np.full(HEADER, np.nan)
    host.sh_header(C.byref(p), C.byref(a), C.byref(cam), got.ctypes.data)
    want = abi_cases.hand_made_state(p, a, cam)[:HEADER]                               # written from the header's comment, field by field
    assert (got.view(np.uint64) == want.view(np.uint64)).all()
    assert got[0] == abi_cases.MAGIC and got[1] == abi_cases.VERSION and (got[31:] == 0).all()
    host.sh_header(C.byref(p), C.byref(a), None, got.ctypes.data)              # without a camera: its fields stay zero
    assert (got[:16].view(np.uint64) == want[:16].view(np.uint64)).all() and (got[16:] == 0).all()


@pytest.mark.parametrize("w,h", [(1, 1), (45, 37), (0, 7), (65535, 65535)])
def test_state_doubles(host, w, h):
    assert host.sh_state_doubles(w, h) == library.product().adaptive_state_doubles(w, h) == HEADER + RECORD * w * h


def _refuse(host, p, a, cam, st, allow_empty=0):
    first, msg = C.c_uint32(77), C.create_string_buffer(512)
    rc = host.sh_refuse(b"render_adaptive_resume", allow_empty, C.byref(p), C.byref(a), C.byref(cam), st.ctypes.data, C.byref(first), msg, 512)
    return rc, msg.value.decode(), first.value


@pytest.mark.parametrize("name,what,msg", STATE_BREAKS, ids=[x[0] for x in STATE_BREAKS])
def test_refusals_are_the_exported_entry_points(host, name, what, msg):
    b = library.product()
    sc = S.Scene(b)
    p, a, cam = abi_cases.params(spp_chunk=4), abi_cases.adaptive(), abi_cases.camera()
    st = abi_cases.break_state(abi_cases.hand_made_state(p, a, cam), what)
    want_rc = _call(b, sc, p, a, state=st)
    want_msg = b.last_error().decode()
    rc, got, _ = _refuse(host, p, a, cam, st)
    assert rc == want_rc == abi_cases.INVALID and got == want_msg and msg in got, (name, got, want_msg)


def test_a_valid_state_passes_and_reports_its_lowest_level(host):
    p, a, cam = abi_cases.params(spp_chunk=4), abi_cases.adaptive(), abi_cases.camera()
    assert _refuse(host, p, a, cam, abi_cases.hand_made_state(p, a, cam)) == (0, "", 1)
    st = abi_cases.hand_made_state(p, a, cam, n=128, k=32)
    assert _refuse(host, p, a, cam, st) == (0, "", 2)
    st[HEADER + 5 * RECORD:HEADER + 6 * RECORD] = 0.0                          # an empty record: the region and budget forms' only
    rc, got, _ = _refuse(host, p, a, cam, st)
    assert rc == abi_cases.INVALID and "below pass_spp" in got
    assert _refuse(host, p, a, cam, st, allow_empty=1) == (0, "", 0)
