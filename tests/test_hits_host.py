"""Hit queries, the part that needs no GPU: the composed CPU reference (hits_helpers) against the restatement's own
Scene::trace, the ABI's new entries, and the one-pixel pinhole ray."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle as orc
from hits_helpers import any_hit, incoherent, kinds
from rays_helpers import NRAYS, SEED, incoherent_rays, oracle_trace, scene
from reflaxman_amd import _lib, cameras

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rfx_query_hits", "rfx_query_hits_host", "rfx_query_occluded", "rfx_query_occluded_host")

# scene: (objects, winners that are spheres / triangles / planes, misses) on incoherent_rays(scene), and the rays
# occluded when each ray leaves out its own winner
EXPECT = {
    "default": (10, [11, 104, 0, 242], 5),
    "planes": (12, [11, 104, 123, 119], 132),
    "synth16_sky": (20, [2, 108, 0, 247], 2),
    "stress4096": (4098, [176, 46, 0, 135], 152),
    "planes300": (304, [68, 101, 86, 102], 159),
    "mesh100": (108, [10, 108, 0, 239], 9),
    "mesh40x32": (2568, [4, 106, 0, 247], 7),
    "soup300": (302, [0, 122, 0, 235], 19),
}


@pytest.mark.parametrize("name", list(EXPECT))
def test_composed_reference_reproduces_scene_trace(name):
    """The composed winners' kinds are the hit counters of the restatement's Scene::trace at depth 1 (one closest-hit
    pass per ray), and equal the recorded numbers; both answers occur at least 100 times."""
    desc = scene(name)
    objects, want, _ = EXPECT[name]
    assert len(desc.objects) == objects
    planes, tab = incoherent(name)
    got = kinds(desc, planes["object"])
    cnt = np.zeros(len(orc.COUNTER_NAMES), np.uint64)
    oracle_trace(desc, incoherent_rays(name), 1, SEED, cnt)
    c = {k: int(cnt[i]) for i, k in enumerate(orc.COUNTER_NAMES)}
    assert got == [c["hit_sph"], c["hit_tri"], c["hit_pln"], c["sky"]], (name, got)
    assert got == want, (name, got)
    assert sum(got) == NRAYS and sum(got[:3]) >= 100 and got[3] >= 100
    miss = planes["object"] < 0
    assert (planes["distance"][miss] == np.float32(3.4028234663852886e38)).all()
    assert np.isfinite(planes["distance"][~miss]).all() and (planes["distance"][~miss] > 0).all()
    for k in ("point", "normal", "reflected", "colour"):
        assert not planes[k][miss].any()


@pytest.mark.parametrize("name", list(EXPECT))
def test_composed_any_hit_depends_on_skip(name):
    """With each ray leaving out its own winner the any-hit has both answers (at least 2 rays each) and differs from
    the no-skip answer on at least 50 rays; without a skip it is `some object is hit`."""
    planes, tab = incoherent(name)
    plain = any_hit(tab)
    own = any_hit(tab, planes["object"])
    assert int(own.sum()) == EXPECT[name][2], (name, int(own.sum()))
    assert own.sum() >= 2 and (own == 0).sum() >= 2
    assert int((own != plain).sum()) >= 50
    assert np.array_equal(any_hit(tab, np.full(NRAYS, len(scene(name).objects))), plain)
    assert np.array_equal(any_hit(tab, np.full(NRAYS, -7)), plain)


def test_header_library_and_binding_have_the_query_entries():
    text = open(os.path.join(ROOT, "include", "rfx.h")).read()
    assert re.search(r"^#define RFX_ABI_VERSION 5$", text, re.M)
    assert re.search(r"\}\s*rfx_hit_planes;", text)
    for field in ("int32_t *object;", "*distance;", "*point;", "*normal;", "*reflected;", "*colour;"):
        assert re.sub(r"\s+", "", field) in re.sub(r"\s+", "", text), field
    L = _lib.load()
    assert L.rfx_abi_version() == 5 and _lib.RFX_ABI_VERSION == 5
    bound = {n for n, _, _ in _lib.SIGNATURES}
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, text) and hasattr(L, name) and name in bound, name
    assert [f for f, _ in _lib.HitPlanes._fields_] == ["object", "distance", "point", "normal", "reflected", "colour"]
    assert C.sizeof(_lib.HitPlanes) == 6 * C.sizeof(C.c_void_p)


def test_null_renderer_is_an_argument_error():
    L = _lib.load()
    rays = np.zeros((4, 6), np.float32)
    obj = np.zeros(4, np.int32)
    occ = np.zeros(4, np.uint8)
    hp = _lib.HitPlanes(object=obj.ctypes.data)
    assert L.rfx_query_hits(None, C.c_void_p(rays.ctypes.data), 4, 0, C.byref(hp), None) == -1
    assert L.rfx_query_hits_host(None, _lib.fptr(rays), 4, 0, C.byref(hp)) == -1
    assert L.rfx_query_occluded(None, C.c_void_p(rays.ctypes.data), None, 4, 0, C.c_void_p(occ.ctypes.data), None) == -1
    assert L.rfx_query_occluded_host(None, _lib.fptr(rays), None, 4, 0, occ.ctypes.data_as(C.POINTER(C.c_uint8))) == -1
    assert not obj.any() and not occ.any()


@pytest.mark.parametrize("W,H", [(16, 12), (7, 3)])
def test_pinhole_ray_is_the_row_of_pinhole_rays(W, H):
    desc = scene("default")
    eye, at, fov = desc.camera
    view = orc.camera_view(eye, at)
    rays = cameras.pinhole_rays(eye, view, fov, W, H)
    for y in range(H):
        for x in range(W):
            one = cameras.pinhole_ray(eye, view, fov, W, H, x, y)
            assert one.dtype == np.float32 and one.shape == (6,)
            assert one.tobytes() == rays[y * W + x].tobytes(), (x, y)
