"""The coherent order, the part that needs no GPU: the ABI's new entries, the key's restatement (order_helpers) on the
rays at its edges against expectations worked out by hand, and the key's quality on a permuted pinhole frame."""
import ctypes as C
import os
import re

import numpy as np

import oracle as orc
from order_helpers import CB, DB, cells, dir_cells, keys, order, scene_box, special_rays
from rays_helpers import scene
from reflaxman_amd import _lib, cameras

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rfx_rays_order", "rfx_rays_order_host", "rfx_trace_rays_ordered", "rfx_query_hits_ordered",
           "rfx_query_occluded_ordered", "rfx_renderer_order_box")
F = np.float32


def test_header_library_and_binding_have_the_order_entries():
    text = open(os.path.join(ROOT, "include", "rfx.h")).read()
    assert re.search(r"^#define RFX_ABI_VERSION 5$", text, re.M)
    macro = lambda name: int(re.search(r"^#define %s (\d+)$" % name, text, re.M).group(1))
    assert macro("RFX_ORDER_CELL_BITS") == _lib.RFX_ORDER_CELL_BITS == CB
    assert macro("RFX_ORDER_DIR_BITS") == _lib.RFX_ORDER_DIR_BITS == DB
    assert macro("RFX_ORDER_TILE") == _lib.RFX_ORDER_TILE and _lib.RFX_ORDER_TILE % 64 == 0
    assert CB >= 1 and DB >= 1 and 3 * CB + 2 * DB <= 32
    L = _lib.load()
    assert L.rfx_abi_version() == 5
    bound = {n for n, _, _ in _lib.SIGNATURES}
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, text) and hasattr(L, name) and name in bound, name


def test_null_renderer_is_an_argument_error():
    L = _lib.load()
    rays = np.zeros((4, 6), np.float32)
    out = np.full(4, 7, np.uint32)
    lo = np.zeros(3, np.float32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    hp = _lib.HitPlanes(object=out.ctypes.data)
    assert L.rfx_rays_order(None, p(rays), 4, p(out), None, None) == -1
    assert L.rfx_rays_order_host(None, _lib.fptr(rays), 4, _lib.u32ptr(out), None) == -1
    assert L.rfx_trace_rays_ordered(None, p(rays), p(out), 4, 4, p(rays), None, None) == -1
    assert L.rfx_query_hits_ordered(None, p(rays), p(out), 4, C.byref(hp), None) == -1
    assert L.rfx_query_occluded_ordered(None, p(rays), None, p(out), 4, p(out), None) == -1
    assert L.rfx_renderer_order_box(None, _lib.fptr(lo), _lib.fptr(lo)) == -1
    assert (out == 7).all() and not rays.any()


def test_box_of_a_description():
    """The restated box: spheres grown by their radii, triangles' vertices, planes left out; no object, no scale."""
    from reflaxman_amd import scenes
    d = scenes.SceneDesc("box", (0.9, 0.9, 1.0, 0.1), ((0.0, 3.0, -8.0), (0.0, 0.5, 0.0), 1.0))
    d.add_plane((0.0, -100.0, 0.0), (0.0, 1.0, 0.0), scenes.METAL, (1.0, 0.0, 1.0), 0.5)
    lo, scale = scene_box(d)
    assert not lo.any() and not scale.any()
    d.add_sphere((1.0, 2.0, 3.0), 0.5, scenes.METAL, (1.0, 0.0, 0.0), 0.5)
    d.add_triangle((-1.5, 2.0, 3.0), (0.0, 2.0, 4.5), (0.0, 2.0, 3.0), scenes.METAL, (0.0, 0.0, 1.0), 0.5)
    lo, scale = scene_box(d)
    assert lo.tolist() == [-1.5, 1.5, 2.5]
    assert scale.tolist() == [float(F(16) / F(3)), 16.0, 8.0]  # hi = (1.5, 2.5, 4.5)


def test_special_rays_take_the_documented_cells():
    """The restatement on the rays at the key's edges, against cells worked out by hand from rfx.h's expressions for
    the box lo = (-1, -2, -3), hi = (3, 2, 5), whose scale is (4, 4, 2) exactly."""
    lo, hi = np.array([-1.0, -2.0, -3.0], F), np.array([3.0, 2.0, 5.0], F)
    scale = (F(1 << CB) / (hi - lo)).astype(F)
    assert CB == 4 and scale.tolist() == [4.0, 4.0, 2.0]
    rays = special_rays(lo, hi)
    assert rays.dtype == np.float32 and rays.shape[1] == 6 and len(rays) >= 30
    k = keys(rays, lo, scale)
    assert k.dtype == np.uint32
    c, uv = cells(rays, lo, scale), dir_cells(rays)
    top, dtop, dmid = (1 << CB) - 1, (1 << DB) - 1, 1 << (DB - 1)
    assert (c <= top).all() and (uv <= dtop).all()
    assert (k >> np.uint32(2 * DB) < (1 << 3 * CB)).all()

    def one(o, d):
        r = np.array([list(o) + list(d)], F)
        return cells(r, lo, scale)[0].tolist(), dir_cells(r)[0].tolist(), int(keys(r, lo, scale)[0])

    nan, inf = np.nan, np.inf
    mid = (1.0, 0.0, 1.0)  # (o - lo) * scale = (8, 8, 8)
    # directions that are no direction: 0 / 0, inf / inf and NaN all end as NaN, which the clamp takes to cell 0
    for d in ((0.0, 0.0, 0.0), (-0.0, -0.0, -0.0), (nan, nan, nan), (inf, inf, inf), (nan, 1.0, 1.0), (1.0, 1.0, nan)):
        assert one(mid, d)[:2] == ([8, 8, 8], [0, 0]), d
    # one infinite component: a = inf, the finite components give +-0 -> the middle cell, the infinite one NaN -> 0
    assert one(mid, (inf, 1.0, 1.0))[1] == [0, dmid]
    assert one(mid, (-inf, 0.0, 0.0))[1] == [0, dmid]
    # dz = -inf < 0 folds: px = py = +0, so q = (1 - 0) * 1 = 1 on both axes, clamped to the last cell
    assert one(mid, (1.0, 2.0, -inf))[1] == [dtop, dtop]
    # origins: NaN takes the 0, +-inf clamps, outside clamps, lo is cell 0 and hi the last cell
    assert one((nan, 0.0, 1.0), (0.3, -0.5, 0.8))[0] == [0, 8, 8]
    assert one((1.0, nan, nan), (0.3, -0.5, 0.8))[0] == [8, 0, 0]
    assert one((inf, 0.0, 1.0), (0.3, -0.5, 0.8))[0] == [top, 8, 8]
    assert one((1.0, -inf, inf), (0.3, -0.5, 0.8))[0] == [8, 0, top]
    assert one(lo - F(10), (0.3, -0.5, 0.8))[0] == [0, 0, 0]
    assert one(hi + F(10), (0.3, -0.5, 0.8))[0] == [top, top, top]
    assert one(lo, (0.3, -0.5, 0.8))[0] == [0, 0, 0]
    assert one(hi, (0.3, -0.5, 0.8))[0] == [top, top, top]  # (hi - lo) * scale = 16, clamped to 15
    assert one(np.nextafter(hi, F(-inf)), (0.3, -0.5, 0.8))[0] == [top, top, top]
    # the axes: +x (1, 0) -> (last, middle); -x -> (0, middle); +y, -y likewise; +z the centre; -z folds the centre
    # (+0, +0) to the corner (1, 1)
    assert one(mid, (1.0, 0.0, 0.0))[1] == [dtop, dmid]
    assert one(mid, (-1.0, 0.0, 0.0))[1] == [0, dmid]
    assert one(mid, (0.0, 1.0, 0.0))[1] == [dmid, dtop]
    assert one(mid, (0.0, -1.0, 0.0))[1] == [dmid, 0]
    assert one(mid, (0.0, 0.0, 1.0))[1] == [dmid, dmid]
    assert one(mid, (0.0, 0.0, -1.0))[1] == [dtop, dtop]
    # dz = -0.0 is not below zero: the upper hemisphere's map, (1, 1, -0) -> (0.5, 0.5) -> cell 1.5 * 2^(DB - 1)
    assert one(mid, (1.0, 1.0, -0.0))[1] == [dmid + dmid // 2, dmid + dmid // 2]
    assert one(mid, (1.0, 1.0, -0.0)) == one(mid, (1.0, 1.0, 0.0))
    # a -0 x under a fold takes the + sign (px < 0 is false): (-0, 1, -2) -> qx = 1 - 1/3, qy = (1 - 0) * 1
    assert one(mid, (-0.0, 1.0, -2.0))[1] == one(mid, (0.0, 1.0, -2.0))[1]
    assert one(mid, (-0.0, 1.0, -2.0))[1][1] == dtop
    # the key's layout: the cell's Morton index above the direction's, x lowest
    assert one((-1.0 + 0.25, -2.0, -3.0), (0.0, 0.0, 1.0))[0] == [1, 0, 0]
    base = one(lo, (-1.0, 0.0, 0.0))[2]              # cells (0, 0, 0), u = 0, v = 2^(DB - 1): bit 2 (DB - 1) + 1
    assert base == 1 << (2 * (DB - 1) + 1)
    assert one((-1.0 + 0.25, -2.0, -3.0), (-1.0, 0.0, 0.0))[2] == base | 1 << (2 * DB)
    assert one((-1.0, -2.0 + 0.25, -3.0), (-1.0, 0.0, 0.0))[2] == base | 2 << (2 * DB)
    assert one((-1.0, -2.0, -3.0 + 0.5), (-1.0, 0.0, 0.0))[2] == base | 4 << (2 * DB)
    assert one((-1.0 + 0.5, -2.0, -3.0), (-1.0, 0.0, 0.0))[2] == base | 8 << (2 * DB)
    # the stable order of equal keys is the index order
    assert order(np.array([5, 1, 5, 1, 0], np.uint32)).tolist() == [4, 1, 3, 0, 2]


def test_key_quality_on_a_permuted_pinhole_frame():
    """The 256 x 144 pinhole rays of the default scene's camera, permuted, then sorted by the restated keys: a run of
    64 sorted rays -- a wave of an ordered call -- touches few of the frame's 8 x 8 tiles.  A condition on the key's
    definition (a retuned key must still meet it), not a timing."""
    W, H = 256, 144
    d = scene("default")
    eye, at, fov = d.camera
    rays = cameras.pinhole_rays(eye, orc.camera_view(eye, at), fov, W, H)
    perm = np.random.default_rng(12).permutation(W * H)
    tile = ((np.arange(W * H) // W) // 8) * (W // 8) + (np.arange(W * H) % W) // 8
    runs = lambda src: np.array([len(set(tile[src[a:a + 64]].tolist())) for a in range(0, W * H, 64)])
    before = runs(perm)
    assert np.median(before) >= 56  # the permuted input: nearly every ray of a run from another tile
    lo, scale = scene_box(d)
    o = order(keys(rays[perm], lo, scale))
    after = runs(perm[o])
    print("tiles per run of 64: permuted median %g; sorted median %g max %d" % (np.median(before), np.median(after), after.max()))
    assert np.median(after) <= 8 and after.max() <= 16, (np.median(after), int(after.max()))
