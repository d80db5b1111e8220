"""Paths, the part that needs no GPU: the ABI's new entries, the binding's struct, the calls' argument checks (made
before a renderer is read or a device touched) and the state word's decode."""
import ctypes as C
import os
import re

import numpy as np

from reflaxman_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rfx_paths_begin", "rfx_paths_step", "rfx_paths_order")
RFX_ERR_ARG, RFX_ERR_STATE = -1, -3
INT32_MAX = 2 ** 31 - 1


def test_header_library_and_binding_have_the_paths_entries():
    text = open(os.path.join(ROOT, "include", "rfx.h")).read()
    assert re.search(r"^#define RFX_ABI_VERSION 5$", text, re.M)
    L = _lib.load()
    assert L.rfx_abi_version() == 5
    bound = {n for n, _, _ in _lib.SIGNATURES}
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, text) and hasattr(L, name) and name in bound, name
    assert re.search(r"\}\s*rfx_paths;", text)


def test_the_struct_is_six_pointers_in_the_header_order():
    text = open(os.path.join(ROOT, "include", "rfx.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*rfx_paths;", text).group(1)
    fields = re.findall(r"\*(d_\w+);", body)
    assert fields == ["d_rays", "d_mul", "d_colour", "d_rand", "d_state", "d_argb"]
    assert [f for f, _ in _lib.PathPlanes._fields_] == fields
    assert C.sizeof(_lib.PathPlanes) == 6 * C.sizeof(C.c_void_p)
    assert all(t is C.c_void_p for _, t in _lib.PathPlanes._fields_)


def planes(**without):
    """Host arrays standing in for the planes (an argument error reads none of them), and the struct on them."""
    a = {k: np.full(24, 7, np.uint32) for k in ("d_rays", "d_mul", "d_colour", "d_rand", "d_state", "d_argb")}
    p = _lib.PathPlanes(**{k: (None if k in without else v.ctypes.data) for k, v in a.items()})
    return a, p


def test_null_renderer_is_an_argument_error():
    L = _lib.load()
    a, p = planes()
    idx = np.full(4, 7, np.uint32)
    q = C.c_void_p(idx.ctypes.data)
    assert L.rfx_paths_begin(None, C.byref(p), 4, 1, None) == RFX_ERR_ARG
    assert L.rfx_paths_step(None, C.byref(p), 4, None, 4, 1, None, None, None) == RFX_ERR_ARG
    assert L.rfx_paths_step(None, C.byref(p), 4, q, 4, 1, q, q, None) == RFX_ERR_ARG
    assert L.rfx_paths_order(None, C.byref(p), 4, None, 4, q, None) == RFX_ERR_ARG
    assert (idx == 7).all() and all((v == 7).all() for v in a.values())


def test_argument_errors_come_before_the_renderer_is_read():
    """Each argument error of rfx.h on a renderer that is none -- zeroed memory, never dereferenced on these paths.  The
    same memory with good arguments reads as a renderer without a scene: RFX_ERR_STATE, so the checks below fail for
    their arguments and nothing else."""
    L = _lib.load()
    fake = C.create_string_buffer(1 << 16)
    r = C.cast(fake, C.c_void_p)
    a, p = planes()
    idx = np.full(4, 7, np.uint32)
    q = C.c_void_p(idx.ctypes.data)
    by = C.byref
    assert L.rfx_paths_step(r, by(p), 4, None, 4, 1, None, None, None) == RFX_ERR_STATE
    assert L.rfx_paths_step(r, by(p), 4, q, 4, 1, q, q, None) == RFX_ERR_STATE
    assert L.rfx_paths_step(r, by(p), 4, None, 4, 1, None, q, None) == RFX_ERR_STATE  # the count alone
    assert L.rfx_paths_step(r, by(p), 4, None, 4, INT32_MAX - 1, None, None, None) == RFX_ERR_STATE
    assert L.rfx_paths_step(r, by(p), 2 ** 32 - 1, None, 4, 1, None, None, None) == RFX_ERR_STATE
    assert L.rfx_paths_begin(r, by(p), 4, 0, None) == RFX_ERR_STATE
    assert L.rfx_paths_order(r, by(p), 4, None, 4, q, None) == RFX_ERR_STATE
    assert L.rfx_paths_step(r, None, 4, None, 4, 1, None, None, None) == RFX_ERR_ARG
    for name in ("d_rays", "d_mul", "d_colour", "d_rand", "d_state"):
        _, bad = planes(**{name: True})
        assert L.rfx_paths_step(r, by(bad), 4, None, 4, 1, None, None, None) == RFX_ERR_ARG, name
        assert L.rfx_paths_begin(r, by(bad), 4, 1, None) == RFX_ERR_ARG, name
    _, no_argb = planes(d_argb=True)
    assert L.rfx_paths_step(r, by(no_argb), 4, None, 4, 1, None, None, None) == RFX_ERR_STATE  # d_argb is optional
    assert L.rfx_paths_step(r, by(p), 4, None, 0, 1, None, None, None) == RFX_ERR_ARG          # slots == 0
    assert L.rfx_paths_step(r, by(p), 0, None, 4, 1, None, None, None) == RFX_ERR_ARG          # n == 0
    assert L.rfx_paths_step(r, by(p), 2 ** 32, None, 4, 1, None, None, None) == RFX_ERR_ARG    # n >= 2^32
    assert L.rfx_paths_step(r, by(p), 4, None, 4, 0, None, None, None) == RFX_ERR_ARG          # upto < 1
    assert L.rfx_paths_step(r, by(p), 4, None, 4, -3, None, None, None) == RFX_ERR_ARG
    assert L.rfx_paths_step(r, by(p), 4, None, 4, INT32_MAX, None, None, None) == RFX_ERR_ARG  # upto == INT32_MAX
    assert L.rfx_paths_step(r, by(p), 4, None, 4, 1, q, None, None) == RFX_ERR_ARG             # a list without a count
    assert L.rfx_paths_begin(r, None, 4, 1, None) == RFX_ERR_ARG
    assert L.rfx_paths_begin(r, by(p), 0, 1, None) == RFX_ERR_ARG
    assert L.rfx_paths_order(r, None, 4, None, 4, q, None) == RFX_ERR_ARG
    assert L.rfx_paths_order(r, by(p), 4, None, 4, None, None) == RFX_ERR_ARG
    assert L.rfx_paths_order(r, by(p), 0, None, 4, q, None) == RFX_ERR_ARG
    assert L.rfx_paths_order(r, by(p), 2 ** 32, None, 4, q, None) == RFX_ERR_ARG
    assert L.rfx_paths_order(r, by(p), 4, None, 0, q, None) == RFX_ERR_ARG
    assert L.rfx_paths_order(r, by(p), 4, None, 2 ** 31, q, None) == RFX_ERR_ARG
    _, no_rays = planes(d_rays=True)
    assert L.rfx_paths_order(r, by(no_rays), 4, None, 4, q, None) == RFX_ERR_ARG
    assert (idx == 7).all() and all((v == 7).all() for v in a.values())
    assert not any(fake.raw)


def test_state_decode_round_trips():
    """s >= 0: live after s segments; s < 0: ended after ~s (>= 1) segments."""
    seg = np.arange(1, 40, dtype=np.int32)
    ended = _lib.path_ended_state(seg)
    assert ended.dtype == np.int32 and (ended < 0).all() and ended[0] == -2 and int(ended[-1]) == -40
    assert np.array_equal(_lib.path_segments(ended), seg)
    live = np.arange(0, 40, dtype=np.int32)
    assert np.array_equal(_lib.path_segments(live), live)
    mixed = np.array([0, 3, -2, -9, INT32_MAX - 1, -INT32_MAX - 1], np.int32)
    assert _lib.path_segments(mixed).tolist() == [0, 3, 1, 8, INT32_MAX - 1, INT32_MAX]
    assert int(_lib.path_segments(np.int32(-2))) == 1 and int(_lib.path_ended_state(1)) == -2
