"""Hit queries on the GPU (rfx.h rfx_query_hits, rfx_query_occluded): the closest hit and the any-hit of rays the
caller chose, against the reference's answers composed on the CPU (hits_helpers).  The bar is bit equality on every
word of every plane, misses included."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle as orc
from helpers import GOLDEN, manifest
from hits_helpers import FLT_MAX, PLANES, any_hit, compose, incoherent, same_bits
from rays_helpers import NRAYS, SEED, incoherent_rays, scene
from reflaxman_amd import _lib, cameras, scenes

pytestmark = pytest.mark.gpu

RFX_ERR_ARG, RFX_ERR_STATE = -1, -3
_DESC = {}


def desc_of(name):
    """A scene description by name: rays_helpers' scenes, and the ones only these tests use."""
    if name not in _DESC:
        if name == "soup300_degenerate":
            _DESC[name] = scenes.degenerate_soup_scene()
        elif name == "mesh100_plane":  # a triangle tree and a plane in one scene
            d = scenes.get_scene("mesh100")
            d.add_plane((0.0, -0.05, 0.0), (0.0, 2.0, 0.0), scenes.DIELECTRIC, (0.8, 0.85, 0.9), 0.6)
            _DESC[name] = d
        elif name in ("ties", "ties_large"):
            _DESC[name] = ties_scene(40 if name == "ties_large" else 0)
        else:
            _DESC[name] = scene(name)
    return _DESC[name]


def ties_scene(fillers):
    """Exact ties: a sphere added twice and a triangle added twice, different colours each time, and a plane coplanar
    with a triangle whose basis is made of powers of two (both give t = -o.y / ray.y exactly).  fillers: small spheres
    added afterwards, which make the scene a large one (its spheres in spatial order on the device)."""
    d = scenes.SceneDesc("ties", (0.9, 0.9, 1.0, 0.1), ((0.0, 3.0, -8.0), (0.0, 0.5, 0.0), 1.0))
    d.add_sphere((-1.5, 1.0, 0.0), 1.0, scenes.METAL, (1.0, 0.0, 0.0), 0.5)
    d.add_sphere((-1.5, 1.0, 0.0), 1.0, scenes.DIELECTRIC, (0.0, 1.0, 0.0), 0.25)
    tri = ((0.5, 0.25, 1.0), (0.75, 2.5, 1.5), (2.5, 0.5, 0.5))
    d.add_triangle(*tri, scenes.METAL, (0.0, 0.0, 1.0), 0.5)
    d.add_triangle(*tri, scenes.DIELECTRIC, (1.0, 1.0, 0.0), 0.75)
    d.add_triangle((-4.0, 0.0, -4.0), (-4.0, 0.0, 4.0), (4.0, 0.0, -4.0), scenes.METAL, (0.0, 1.0, 1.0), 0.5)
    d.add_plane((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), scenes.METAL, (1.0, 0.0, 1.0), 0.5)
    for k in range(fillers):
        d.add_sphere((-6.0 + 0.3 * k, 0.2 + 0.05 * (k % 7), 3.0 - 0.1 * k), 0.15, scenes.METAL, (0.5, 0.5, 0.5), 0.5)
    return d


def renderer(name, tri_accel=None):
    """(Renderer with the scene uploaded, its Scene -- kept alive by the caller --, the scene's Camera)."""
    from reflaxman_amd.render import Renderer, build_scene
    s, cam = build_scene(desc_of(name))
    r = Renderer(sphere_seed=SEED, jitter_seed=77)
    if tri_accel is not None:
        r.set_tri_accel(tri_accel)
    r.set_scene(s)
    return r, s, cam


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared references are read-only)


def hits(r, rays, **kw):
    """Renderer.query_hits' device form on a side stream, the planes back as numpy."""
    import torch
    with torch.cuda.stream(torch.cuda.Stream()):
        out = r.query_hits(dev(rays), **kw)
        torch.cuda.current_stream().synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def shadow(r, rays, skip=None, **kw):
    import torch
    with torch.cuda.stream(torch.cuda.Stream()):
        out = r.occluded(dev(rays), None if skip is None else dev(np.asarray(skip, np.int32)), **kw)
        torch.cuda.current_stream().synchronize()
    return out.cpu().numpy()


def assert_planes(got, want, tag):
    for k in got:
        bad = same_bits(got[k], want[k])
        assert bad.size == 0, (tag, k, bad[:8].tolist(), got[k][bad[:2]].tolist(), want[k][bad[:2]].tolist())


def pinhole(name, W, H):
    d = desc_of(name)
    eye, at, fov = d.camera
    return cameras.pinhole_rays(eye, orc.camera_view(eye, at), fov, W, H)


# the scenes only these tests use take the rays of the scene they grew from
RAYS_OF = {"soup300_degenerate": "soup300", "mesh100_plane": "mesh100"}
# (scene, tri_accel, the triangle tree the case is meant to run with: None = whatever the scene gives)
INCOHERENT = [("default", None, None), ("planes", None, None), ("synth16_sky", None, None), ("stress4096", None, None),
              ("planes300", None, None), ("mesh100", None, None), ("mesh40x32", None, None), ("soup300", None, None),
              ("mesh100", -1, False), ("mesh100", 1, True), ("mesh40x32", -1, True), ("mesh40x32", 2, True),
              ("soup300_degenerate", 1, True), ("mesh100_plane", 1, True)]


@pytest.mark.parametrize("name,tri_accel,tree", INCOHERENT)
def test_incoherent_rays_equal_the_composed_reference(name, tri_accel, tree):
    """357 rays with nothing in common, all six planes, as a linear batch and as rasters 21 wide (partial tiles in x,
    17 full rows) and 24 wide (W % 4 == 0, a partial last row); the any-hit with nothing left out, and with each ray
    leaving out its own winner."""
    rays = incoherent_rays(RAYS_OF.get(name, name))
    want, tab = compose(desc_of(name), rays, key=("incoherent", name))
    r, s, cam = renderer(name, tri_accel)
    info = r.accel_info()
    if tree is not None:
        assert (info.tri_nodes > 0) == tree, (name, tri_accel, info.tri_nodes)
    if tri_accel == 2:
        assert info.narrow_tri_bvh
    if name == "soup300_degenerate":
        assert info.tri_residual > 0
    for rw in (0, 21, 24):
        got = hits(r, rays, raster_width=rw)
        assert sorted(got) == sorted(PLANES)
        assert_planes(got, want, (name, tri_accel, rw))
        occ = shadow(r, rays, raster_width=rw)
        assert np.array_equal(occ, any_hit(tab)), (name, rw, np.flatnonzero(occ != any_hit(tab))[:8].tolist())
        assert np.array_equal(occ, (got["object"] >= 0).astype(np.uint8))
        own = shadow(r, rays, want["object"], raster_width=rw)
        ref = any_hit(tab, want["object"])
        assert np.array_equal(own, ref), (name, rw, np.flatnonzero(own != ref)[:8].tolist())
    r.close()


@pytest.mark.parametrize("name,tri_accel", [("default", None), ("stress4096", None), ("mesh40x32", None),
                                            ("soup300_degenerate", 1)])
def test_coherent_rays(name, tri_accel):
    """A 40 x 24 pinhole frame's rays -- narrow bundles: the wave-wide culls -- as a raster and as a linear batch."""
    rays = pinhole(name, 40, 24)
    want, tab = compose(desc_of(name), rays, key=("pinhole", name))
    assert (want["object"] >= 0).sum() >= 100
    r, s, cam = renderer(name, tri_accel)
    for rw in (40, 0):
        assert_planes(hits(r, rays, raster_width=rw), want, (name, rw))
        assert np.array_equal(shadow(r, rays, raster_width=rw), any_hit(tab)), (name, rw)
        own = shadow(r, rays, want["object"], raster_width=rw)
        assert np.array_equal(own, any_hit(tab, want["object"])), (name, rw)
    r.close()


@pytest.mark.parametrize("name", ["default", "stress4096"])
def test_sizes_and_splitting(name):
    """Batches of 1, 63, 64 and 65 rays are prefixes of the 357-ray result; with the launch limit at one wave
    (linear) or one tile row (raster) the batch runs as many launches and no output changes."""
    rays = incoherent_rays(name)
    want, tab = incoherent(name)
    r, s, cam = renderer(name)
    for n in (1, 63, 64, 65):
        for rw in (0, 8):
            assert_planes(hits(r, rays[:n], raster_width=rw), {k: v[:n] for k, v in want.items()}, (name, n, rw))
            assert np.array_equal(shadow(r, rays[:n], want["object"][:n], raster_width=rw),
                                  any_hit(tab, want["object"])[:n]), (name, n, rw)
    for limit, rws in ((64, (0,)), (1, (0, 8, 24))):
        r.set_launch_traces(limit)
        for rw in rws:
            assert_planes(hits(r, rays, raster_width=rw), want, (name, "split", limit, rw))
            assert np.array_equal(shadow(r, rays, want["object"], raster_width=rw), any_hit(tab, want["object"]))
    r.close()


def test_planes_alone_sentinels_and_alignment():
    """Each plane requested alone equals itself requested with the others; 16 sentinel words either side of every
    buffer stay as they were, an unrequested buffer stays wholly as it was; plane pointers that are 4-B aligned only
    give the same values."""
    import torch
    L = _lib.load()
    name = "planes300"
    rays = incoherent_rays(name)
    want, _ = incoherent(name)
    r, s, cam = renderer(name)
    for k in PLANES:
        assert_planes(hits(r, rays, want=(k,)), {k: want[k]}, (name, "alone", k))
    d_rays = dev(rays)
    SENT, PAD = 0x5A5A5A5A, 16
    words = {k: NRAYS * (1 if k in ("object", "distance") else 3) for k in PLANES}
    for off, asked in ((0, PLANES), (1, PLANES), (0, ("object", "normal")), (1, ("distance", "colour"))):
        buf = {k: torch.full((PAD + off + words[k] + PAD,), SENT, dtype=torch.int32, device="cuda") for k in PLANES}
        torch.cuda.synchronize()  # the renderer's own stream is not ordered with torch's
        hp = _lib.HitPlanes()
        for k in asked:
            setattr(hp, k, buf[k].data_ptr() + 4 * (PAD + off))
        _lib.check(L.rfx_query_hits(r._h, C.c_void_p(d_rays.data_ptr()), NRAYS, 24 if off else 0, C.byref(hp), None))
        r.synchronize()
        for k in PLANES:
            b = buf[k].cpu().numpy()
            if k not in asked:
                assert (b == SENT).all(), (k, off, asked)
                continue
            assert (b[:PAD + off] == SENT).all() and (b[PAD + off + words[k]:] == SENT).all(), (k, off)
            got = b[PAD + off:PAD + off + words[k]].view(want[k].dtype).reshape(want[k].shape)
            assert same_bits(got, want[k]).size == 0, (k, off, asked)
    r.close()


@pytest.mark.parametrize("name", ["ties", "ties_large"])
def test_ties_go_to_the_lower_index(name):
    """Among equal distances the lowest object index wins (Scene.cpp:98: strict `<` in insertion order): the copy
    added second never wins, the coplanar plane never beats its triangle, and the colour is the winner's."""
    d = desc_of(name)
    rays = pinhole(name, 24, 16)
    want, tab = compose(d, rays, key=("pinhole", name))
    hit = tab[:, :, 0] > 0
    dist = tab[:, :, 10]
    for a, b in ((0, 1), (2, 3)):  # the twins hit together, at one distance
        assert np.array_equal(hit[a], hit[b]) and hit[a].sum() >= 10
        assert np.array_equal(dist[a][hit[a]], dist[b][hit[a]])
    both = hit[4] & hit[5]
    assert both.sum() >= 10 and np.array_equal(dist[4][both], dist[5][both])  # the plane ties with its triangle
    won = set(want["object"].tolist())
    assert {0, 2, 4, 5} <= won and not ({1, 3} & won)
    assert not ((want["object"] == 5) & hit[4]).any()
    r, s, cam = renderer(name)
    info = r.accel_info()
    assert (info.sph_nodes > 0) == (name == "ties_large")
    for rw in (24, 0):
        got = hits(r, rays, raster_width=rw)
        assert_planes(got, want, (name, rw))
        for obj, rgb in ((0, (1.0, 0.0, 0.0)), (2, (0.0, 0.0, 1.0)), (4, (0.0, 1.0, 1.0))):
            assert (got["colour"][got["object"] == obj] == np.array(rgb, np.float32)).all(), (name, obj)
        assert np.array_equal(shadow(r, rays, want["object"], raster_width=rw), any_hit(tab, want["object"]))
    r.close()


def test_queries_leave_the_renderer_state_alone():
    """The random streams read the same before and after; a frame rendered after queries is the golden frame, and so
    is the still view's second frame (rendered with the per-view masks held) with queries in between; a rewind after
    "frame, then query" succeeds."""
    from reflaxman_amd.render import Render, build_scene
    key = "render_default_160x120_d4"
    c = manifest()["cases"][key]
    g = np.load(os.path.join(GOLDEN, key + ".npz"))
    W, H, depth = c["W"], c["H"], c["depth"]
    o = orc.OracleRender(scene("default"), c["sphere_seed"], 0)
    o.set_image_size(W, H)
    o.render(depth, 1)
    assert o.image.tobytes() == g["rgb"].tobytes()
    seed1 = o.sphere_seed.value
    o.render(depth, 1)
    rays = incoherent_rays("default")
    want, tab = incoherent("default")
    R = Render(sphere_seed=c["sphere_seed"], jitter_seed=0, load_default_scene=False)
    R.scene, R.camera = build_scene(scene("default"))
    R.setImageSize(W, H)
    r = R._r
    r.set_scene(R.scene)

    def frame():
        R.renderBegin(depth, 1, False)
        while R.renderNext(W * H):
            pass

    assert_planes(hits(r, rays), want, "before")
    assert np.array_equal(shadow(r, rays), any_hit(tab))
    assert r.get_rng() == (c["sphere_seed"], 0)
    frame()
    R.synchronize()
    assert R.image.tobytes() == g["rgb"].tobytes()
    assert r.get_rng() == (seed1, 0)
    assert_planes(hits(r, rays, raster_width=24), want, "between")
    assert np.array_equal(shadow(r, rays, want["object"]), any_hit(tab, want["object"]))
    assert r.get_rng() == (seed1, 0)
    frame()
    R.synchronize()
    assert R.image.tobytes() == o.image.tobytes()
    assert r.get_rng() == (o.sphere_seed.value, 0)
    # frame, then query, then the rewind: the streams return to the frame's start
    assert_planes(r.query_hits(rays), want, "host form")
    assert _lib.load().rfx_frame_rng_rewind(r._h) == 0
    assert r.get_rng() == (seed1, 0)
    R.close()


def test_errors():
    import torch
    from reflaxman_amd.render import Renderer
    L = _lib.load()
    rays = dev(incoherent_rays("default")[:64])
    obj = torch.zeros(64, dtype=torch.int32, device="cuda")
    occ = torch.zeros(64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p = lambda t: C.c_void_p(t.data_ptr())
    hp, none = _lib.HitPlanes(object=obj.data_ptr()), _lib.HitPlanes()
    bare = Renderer(sphere_seed=SEED)
    assert L.rfx_query_hits(bare._h, p(rays), 64, 0, C.byref(hp), None) == RFX_ERR_STATE  # no scene
    assert L.rfx_query_occluded(bare._h, p(rays), None, 64, 0, p(occ), None) == RFX_ERR_STATE
    bare.close()
    r, s, cam = renderer("default")
    assert L.rfx_query_hits(r._h, p(rays), 0, 0, C.byref(hp), None) == RFX_ERR_ARG
    assert L.rfx_query_hits(r._h, None, 64, 0, C.byref(hp), None) == RFX_ERR_ARG
    assert L.rfx_query_hits(r._h, p(rays), 64, 0, None, None) == RFX_ERR_ARG
    assert L.rfx_query_hits(r._h, p(rays), 64, 0, C.byref(none), None) == RFX_ERR_ARG
    assert L.rfx_query_hits(None, p(rays), 64, 0, C.byref(hp), None) == RFX_ERR_ARG
    assert L.rfx_query_occluded(r._h, p(rays), None, 0, 0, p(occ), None) == RFX_ERR_ARG
    assert L.rfx_query_occluded(r._h, None, None, 64, 0, p(occ), None) == RFX_ERR_ARG
    assert L.rfx_query_occluded(r._h, p(rays), None, 64, 0, None, None) == RFX_ERR_ARG
    host = np.zeros(64, np.uint8)
    assert L.rfx_query_hits_host(r._h, None, 64, 0, C.byref(hp)) == RFX_ERR_ARG
    assert L.rfx_query_occluded_host(r._h, None, None, 64, 0, host.ctypes.data_as(C.POINTER(C.c_uint8))) == RFX_ERR_ARG
    assert L.rfx_query_hits(r._h, p(rays), 64, 0, C.byref(hp), None) == 0
    r.synchronize()
    with pytest.raises(ValueError):
        r.query_hits(rays, want=("depth",))
    with pytest.raises(ValueError):
        r.query_hits(rays, want=())
    r.close()


@pytest.mark.parametrize("name", ["planes", "planes300"])
def test_any_hit_skip_values_and_host_form(name):
    """A skip outside [0, objects) leaves nothing out; the host forms agree with the device forms."""
    rays = incoherent_rays(name)
    want, tab = incoherent(name)
    r, s, cam = renderer(name)
    plain = shadow(r, rays)
    assert np.array_equal(plain, any_hit(tab))
    for v in (len(desc_of(name).objects), -7, 2 ** 30):
        assert np.array_equal(shadow(r, rays, np.full(NRAYS, v, np.int32)), plain), v
    own = any_hit(tab, want["object"])
    assert np.array_equal(r.occluded(rays, want["object"]), own)
    assert np.array_equal(r.occluded(rays, raster_width=24), plain)
    assert np.array_equal(shadow(r, rays, want["object"]), own)
    assert_planes(r.query_hits(rays, raster_width=21), want, (name, "host"))
    assert_planes(r.query_hits(rays, want=("distance", "reflected")),
                  {k: want[k] for k in ("distance", "reflected")}, (name, "host, two planes"))
    r.close()


def test_render_pick():
    """Render.pick under five pixels of the default scene at 160 x 120 -- a sphere, the textured ground, the sky and
    two corners -- equals the composed reference for that pixel's pinhole ray."""
    from reflaxman_amd.render import Render, build_scene
    d = scene("default")
    W, H = 160, 120
    eye, at, fov = d.camera
    view = orc.camera_view(eye, at)
    frame = cameras.pinhole_rays(eye, view, fov, W, H)
    want, _ = compose(d, frame, key=("pinhole160", "default"))
    obj = want["object"].reshape(H, W)
    kind = np.array([{"sphere": 0, "triangle": 1, "plane": 2}[ob[0]] for ob in d.objects])
    first = lambda mask: tuple(int(v) for v in np.argwhere(mask)[len(np.argwhere(mask)) // 2][::-1])
    picks = [first((obj >= 0) & (kind[np.maximum(obj, 0)] == 0)), first((obj >= 0) & (kind[np.maximum(obj, 0)] == 1)),
             first(obj < 0), (0, 0), (W - 1, H - 1)]
    assert kind[obj[picks[0][1], picks[0][0]]] == 0 and kind[obj[picks[1][1], picks[1][0]]] == 1
    R = Render(sphere_seed=SEED, jitter_seed=77, load_default_scene=False)
    R.scene, R.camera = build_scene(d)
    R.setImageSize(W, H)
    for (x, y) in picks:
        one = cameras.pinhole_ray(eye, view, fov, W, H, x, y)
        assert one.tobytes() == frame[y * W + x].tobytes()
        o, dist = R.pick(x, y)
        i = y * W + x
        assert o == int(want["object"][i]), (x, y)
        assert np.float32(dist).tobytes() == want["distance"][i].tobytes(), (x, y)
    assert R.pick(*picks[2]) == (-1, float(FLT_MAX))
    with pytest.raises(ValueError):
        R.pick(W, 0)
    assert R.getRng() == (SEED, 77)
    R.close()
