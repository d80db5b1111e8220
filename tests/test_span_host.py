"""Span queries, the part that needs no GPU: the ray sets that make the GPU tests mean something (span_helpers), the
composed layers against their definition, and the ABI's new entries."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from hits_helpers import closest
from span_helpers import band_pairs, composed, counts, layers, pierce

from reflaxman_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rfx_query_hits_span", "rfx_query_occluded_span", "rfx_query_hits_span_ordered",
           "rfx_query_occluded_span_ordered", "rfx_query_hits_span_host", "rfx_query_occluded_span_host")

# scene: pierce rays with a second candidate, with a fourth
EXPECT = {
    "default": (279, 9),
    "planes": (357, 221),
    "synth16_sky": (292, 16),
    "stress4096": (357, 345),
    "planes300": (357, 310),
    "mesh100": (49, 0),
    "mesh40x32": (78, 14),
    "soup300": (289, 28),
}
# scene: far(pierce, 1e6) rays whose two nearest distances lie within 2^-20 relative, and are one float; the floors
EXPECT_FAR = {
    "default": (60, 7, 50, 5),
    "planes": (57, 7, 50, 5),
    "stress4096": (130, 23, 50, 5),
    "soup300": (32, 1, 25, 0),
}


@pytest.mark.parametrize("name", list(EXPECT))
def test_pierce_rays_have_layers(name):
    """Every pierce ray hits, at least 40 have a second candidate; the counts are the recorded ones."""
    planes, tab, col = pierce(name)
    c = counts(tab)
    assert (planes["object"] >= 0).all() and (c >= 1).all()
    got = (int((c >= 2).sum()), int((c >= 4).sum()))
    assert got[0] >= 40
    assert got == EXPECT[name], (name, got)


@pytest.mark.parametrize("name", list(EXPECT_FAR))
def test_far_rays_crowd_the_band(name):
    """From 1e6 behind, the two nearest distances of many rays fall inside tri_takes' 2^-20 band, some on one float."""
    planes, tab, col = composed(name, "far")
    band, same, band_floor, same_floor = EXPECT_FAR[name]
    got = band_pairs(tab)
    assert got[0] >= band_floor and got[1] >= same_floor, (name, got)
    assert got == (band, same), (name, got)


@pytest.mark.parametrize("name,kind", [(n, "pierce") for n in EXPECT] + [(n, "far") for n in EXPECT_FAR])
def test_layers_follow_their_definition(name, kind):
    """Layer 1 is hits_helpers.closest; a ray's layers ascend strictly in (dist, index); their number is the ray's
    candidate count, and every later layer is a miss."""
    planes, tab, col = composed(name, kind)
    c = counts(tab)
    k = int(min(c.max(), 6)) + 1
    ls = layers(tab, col, k)
    first = closest(tab, col)
    for p in first:
        assert ls[0][p].tobytes() == first[p].tobytes(), (name, p)
    n = tab.shape[1]
    for l in range(k):
        hit = ls[l]["object"] >= 0
        assert np.array_equal(hit, c > l), (name, l)
        ar = np.flatnonzero(hit)
        obj = ls[l]["object"][ar]
        assert (tab[obj, ar, 0] > 0).all() and np.array_equal(tab[obj, ar, 10], ls[l]["distance"][ar])
        miss = ~hit
        assert (ls[l]["distance"][miss] == np.float32(3.4028234663852886e38)).all()
        for p in ("point", "normal", "reflected", "colour"):
            assert not ls[l][p][miss].any()
        if l:
            d0, d1 = ls[l - 1]["distance"][ar], ls[l]["distance"][ar]
            o0, o1 = ls[l - 1]["object"][ar], obj
            assert ((d1 > d0) | ((d1 == d0) & (o1 > o0))).all(), (name, l)
    assert n == c.size


def test_header_library_and_binding_have_the_span_entries():
    text = open(os.path.join(ROOT, "include", "rfx.h")).read()
    assert re.search(r"^#define RFX_ABI_VERSION 5$", text, re.M)
    assert re.search(r"\}\s*rfx_ray_span;", text)
    flat = re.sub(r"\s+", "", text)
    for field in ("const float *d_lo;", "const int32_t *d_after;", "const float *d_hi;"):
        assert re.sub(r"\s+", "", field) in flat, field
    bound = {n for n, _, _ in _lib.SIGNATURES}
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in bound, name
    assert [f for f, _ in _lib.RaySpan._fields_] == ["d_lo", "d_after", "d_hi"]
    assert C.sizeof(_lib.RaySpan) == 3 * C.sizeof(C.c_void_p)


def test_library_exports_the_span_entries():
    L = C.CDLL(_lib.lib_path()) if os.path.exists(_lib.lib_path()) else _lib.load()
    for name in ENTRIES:
        assert hasattr(L, name), name
    L = _lib.load()
    assert L.rfx_abi_version() == 5 and _lib.RFX_ABI_VERSION == 5


def test_null_renderer_is_an_argument_error():
    L = _lib.load()
    rays = np.zeros((4, 6), np.float32)
    obj = np.zeros(4, np.int32)
    occ = np.zeros(4, np.uint8)
    order = np.arange(4, dtype=np.uint32)
    hp = _lib.HitPlanes(object=obj.ctypes.data)
    sp = _lib.RaySpan()
    p = lambda a: C.c_void_p(a.ctypes.data)
    u8 = occ.ctypes.data_as(C.POINTER(C.c_uint8))
    assert L.rfx_query_hits_span(None, p(rays), C.byref(sp), 4, 0, C.byref(hp), None) == -1
    assert L.rfx_query_hits_span(None, p(rays), None, 4, 0, C.byref(hp), None) == -1
    assert L.rfx_query_occluded_span(None, p(rays), None, C.byref(sp), 4, 0, p(occ), None) == -1
    assert L.rfx_query_hits_span_ordered(None, p(rays), C.byref(sp), p(order), 4, C.byref(hp), None) == -1
    assert L.rfx_query_occluded_span_ordered(None, p(rays), None, C.byref(sp), p(order), 4, p(occ), None) == -1
    assert L.rfx_query_hits_span_host(None, _lib.fptr(rays), C.byref(sp), 4, 0, C.byref(hp)) == -1
    assert L.rfx_query_occluded_span_host(None, _lib.fptr(rays), None, C.byref(sp), 4, 0, u8) == -1
    assert not obj.any() and not occ.any()
