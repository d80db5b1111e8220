"""Span queries on the GPU (rfx.h "Ray intervals": rfx_query_hits_span, rfx_query_occluded_span, their ordered and
host forms; Renderer.query_layers, Renderer.visible, Render.pick's layer) against the reference's answers composed on
the CPU (span_helpers).  The bar is bit equality on every word of every requested plane."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle as orc
from helpers import GOLDEN, manifest
from hits_helpers import FLT_MAX, PLANES, same_bits
from rays_helpers import SEED, incoherent_rays, scene
from reflaxman_amd import _lib, cameras, scenes
from span_helpers import INT32_MAX, any_hit_span, closest_span, composed, counts, far, layers, pierce_rays

pytestmark = pytest.mark.gpu

RFX_ERR_ARG, RFX_ERR_STATE = -1, -3
INF = np.float32(np.inf)
SCENES = ("default", "planes", "synth16_sky", "stress4096", "planes300", "mesh100", "mesh40x32", "soup300")
_DESC = {}


def ties_scene(fillers):
    """Exact ties: a sphere added twice and a triangle added twice, different colours each time, and a plane coplanar
    with a triangle whose basis is made of powers of two (both give t = -o.y / ray.y exactly).  fillers: small spheres
    added afterwards, which make the scene a large one."""
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


def desc_of(name):
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


# the scenes only these tests use take the rays of the scene they grew from
RAYS_OF = {"soup300_degenerate": "soup300", "mesh100_plane": "mesh100"}


def ref(name, kind):
    """(rays, closest planes, table, colours) of a scene's "pierce", "far" or "incoherent" rays, composed once."""
    base = RAYS_OF.get(name, name)
    rays = {"pierce": lambda: pierce_rays(base), "far": lambda: far(pierce_rays(base), 1e6),
            "incoherent": lambda: incoherent_rays(base)}[kind]()
    planes, tab, col = composed(name, kind, desc=desc_of(name), rays=rays)
    return rays, planes, tab, col


def renderer(name, tri_accel=None):
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


def assert_occ(got, want, tag):
    assert got.dtype == np.uint8 and np.array_equal(got, want), (tag, np.flatnonzero(got != want)[:8].tolist())


def raw(r, rays, span, any_hit_call=False, skip=None, rw=0, order=None, want=PLANES):
    """The C entries themselves on the renderer's own stream: span is None (a NULL pointer) or a _lib.RaySpan."""
    import torch
    L = _lib.load()
    n = len(rays)
    d_rays = dev(rays)
    p = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)
    sp = C.byref(span) if span is not None else None
    d_order = dev(np.asarray(order, np.uint32).view(np.int32)) if order is not None else None
    if any_hit_call:
        occ = torch.zeros(n, dtype=torch.uint8, device="cuda")
        d_skip = dev(np.asarray(skip, np.int32)) if skip is not None else None
        torch.cuda.synchronize()
        if order is not None:
            _lib.check(L.rfx_query_occluded_span_ordered(r._h, p(d_rays), p(d_skip), sp, p(d_order), n, p(occ), None))
        else:
            _lib.check(L.rfx_query_occluded_span(r._h, p(d_rays), p(d_skip), sp, n, rw, p(occ), None))
        r.synchronize()
        return occ.cpu().numpy()
    out = {k: torch.zeros((n,) if k in ("object", "distance") else (n, 3),
                          dtype=torch.int32 if k == "object" else torch.float32, device="cuda") for k in want}
    hp = _lib.HitPlanes(**{k: out[k].data_ptr() for k in want})
    torch.cuda.synchronize()
    if order is not None:
        _lib.check(L.rfx_query_hits_span_ordered(r._h, p(d_rays), sp, p(d_order), n, C.byref(hp), None))
    else:
        _lib.check(L.rfx_query_hits_span(r._h, p(d_rays), sp, n, rw, C.byref(hp), None))
    r.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def below(x):
    return np.nextafter(np.asarray(x, np.float32), np.float32(0.0)).astype(np.float32)


def above(x):
    with np.errstate(over="ignore"):  # (FLT_MAX goes to +inf)
        return np.nextafter(np.asarray(x, np.float32), INF).astype(np.float32)


def second_distance(tab, col):
    """Each ray's second layer distance, +inf where it has none."""
    l2 = layers(tab, col, 2)[1]
    return np.where(l2["object"] >= 0, l2["distance"], INF).astype(np.float32)


# ------------------------------------------------------------------ no bounds is the old query
@pytest.mark.parametrize("name", SCENES)
def test_no_bounds_is_the_old_query(name):
    """span NULL, a span of NULL arrays, lo = -1 with hi = +inf, and hi = FLT_MAX give rfx_query_hits' and
    rfx_query_occluded's words: linear, as rasters 21 and 24 wide, and ordered (the coherent order)."""
    r, s, cam = renderer(name)
    for kind in ("incoherent", "pierce"):
        rays, want, tab, col = ref(name, kind)
        n = len(rays)
        old = hits(r, rays)
        assert_planes(old, want, (name, kind, "rfx_query_hits"))
        old_occ = shadow(r, rays)
        old_own = shadow(r, rays, want["object"])
        assert_occ(old_occ, any_hit_span(tab), (name, kind, "composed any-hit, out-parameter form"))
        assert_occ(old_own, any_hit_span(tab, want["object"]), (name, kind, "composed, own winner skipped"))
        order = r.order_rays(rays)
        for rw, o in ((0, None), (21, None), (24, None), (0, order)):
            tag = (name, kind, rw, o is not None)
            for span in (None, _lib.RaySpan()):
                assert_planes(raw(r, rays, span, rw=rw, order=o), old, tag + ("NULL", span is None))
                assert_occ(raw(r, rays, span, True, rw=rw, order=o), old_occ, tag)
                assert_occ(raw(r, rays, span, True, want["object"], rw=rw, order=o), old_own, tag)
            kw = dict(raster_width=rw, order=o)
            for lo, hi in ((np.full(n, -1.0, np.float32), np.full(n, INF)), (None, np.full(n, FLT_MAX)),
                           (np.full(n, -1.0, np.float32), None)):
                assert_planes(hits(r, rays, lo=lo, hi=hi, **kw), old, tag + ("wide",))
                assert_occ(shadow(r, rays, lo=lo, hi=hi, **kw), old_occ, tag)
                assert_occ(shadow(r, rays, want["object"], lo=lo, hi=hi, **kw), old_own, tag)
    r.close()


# ------------------------------------------------------------------ the two ends
@pytest.mark.parametrize("name", SCENES)
def test_upper_end(name):
    """hi = the winner's distance keeps the winner (the end is inclusive); one float below it is a miss unless another
    candidate lies there; a per-ray hi either side of the distance gives both outcomes."""
    r, s, cam = renderer(name)
    for kind in ("pierce", "incoherent"):
        rays, want, tab, col = ref(name, kind)
        dist = want["distance"]
        got = hits(r, rays, hi=dist)
        assert_planes(got, want, (name, kind, "hi = dist"))
        lower = below(dist)
        w = closest_span(tab, col, hi=lower)
        assert (w["object"] != want["object"])[want["object"] >= 0].all()  # (dist, winner) itself is gone
        assert_planes(hits(r, rays, hi=lower, raster_width=21), w, (name, kind, "hi below dist"))
        g = np.random.default_rng(20261022)
        with np.errstate(over="ignore"):  # (a miss's FLT_MAX times more than 1 is +inf)
            hi = (dist.astype(np.float64) * 10.0 ** g.uniform(-0.6, 0.6, len(rays))).astype(np.float32)
        w = closest_span(tab, col, hi=hi)
        if kind == "pierce":
            assert (w["object"] >= 0).sum() >= 50 and (w["object"] < 0).sum() >= 50
        assert_planes(hits(r, rays, hi=hi), w, (name, kind, "hi around dist"))
        assert_planes(hits(r, rays, hi=hi, order="coherent"), w, (name, kind, "hi around dist, ordered"))
    r.close()


@pytest.mark.parametrize("name", SCENES)
def test_lower_end(name):
    """(dist, -1) keeps the winner, (dist, winner) gives layer 2, (dist, INT32_MAX) the next strictly farther
    candidate, and so does lo one float above dist."""
    r, s, cam = renderer(name)
    for kind in ("pierce", "incoherent"):
        rays, want, tab, col = ref(name, kind)
        n = len(rays)
        dist, win = want["distance"], want["object"]
        assert_planes(hits(r, rays, lo=dist, after=np.full(n, -1, np.int32)), want, (name, kind, "after = -1"))
        assert_planes(hits(r, rays, lo=dist), want, (name, kind, "after left out"))
        l2 = layers(tab, col, 2)[1]
        w = closest_span(tab, col, lo=dist, after=win)
        assert_planes(w, l2, (name, kind, "the composed references agree"))
        assert_planes(hits(r, rays, lo=dist, after=win, raster_width=24), l2, (name, kind, "layer 2"))
        w = closest_span(tab, col, lo=dist, after=np.full(n, INT32_MAX))
        hit = w["object"] >= 0
        assert (w["distance"][hit] > dist[hit]).all()
        assert_planes(hits(r, rays, lo=dist, after=np.full(n, INT32_MAX)), w, (name, kind, "after = INT32_MAX"))
        assert_planes(hits(r, rays, lo=above(dist), order="coherent"), w, (name, kind, "lo above dist"))
    r.close()


# ------------------------------------------------------------------ layers
LAYERED = [(n, None) for n in SCENES] + \
          [(n, a) for n in ("mesh100", "mesh40x32", "soup300", "soup300_degenerate") for a in (0, 1, 2)] + \
          [("mesh100_plane", 1)]


@pytest.mark.parametrize("name,tri_accel", LAYERED)
def test_four_layers(name, tri_accel):
    """query_layers(pierce, 4) is the first four candidates of every ray in ascending (dist, index)."""
    rays, want, tab, col = ref(name, "pierce")
    ls = layers(tab, col, 4)
    r, s, cam = renderer(name, tri_accel)
    info = r.accel_info()
    if tri_accel is not None:
        assert (info.tri_nodes > 0) == (tri_accel > 0), (name, tri_accel, info.tri_nodes)
    if tri_accel == 2:
        assert info.narrow_tri_bvh
    if name == "stress4096":
        assert info.sph_nodes > 0
    if name == "soup300_degenerate" and tri_accel:
        assert info.tri_residual > 0
    import torch
    with torch.cuda.stream(torch.cuda.Stream()):
        got = r.query_layers(dev(rays), 4)
        torch.cuda.current_stream().synchronize()
    assert len(got) == 4
    for l in range(4):
        assert_planes({k: v.cpu().numpy() for k, v in got[l].items()}, ls[l], (name, tri_accel, "layer", l))
    host = r.query_layers(rays, 3, want=("object", "colour"), raster_width=21)
    for l in range(3):
        assert sorted(host[l]) == ["colour", "object"]
        assert_planes(host[l], {k: ls[l][k] for k in host[l]}, (name, tri_accel, "host layer", l))
    r.close()


def pinhole(name, W, H):
    d = desc_of(name)
    eye, at, fov = d.camera
    return cameras.pinhole_rays(eye, orc.camera_view(eye, at), fov, W, H)


@pytest.mark.parametrize("name", ["ties", "ties_large"])
def test_exact_ties_step_one_object_at_a_time(name):
    """Twins at one distance come as consecutive layers, lower index first, each with its own colour; a lower end that
    excludes the distance skips both."""
    d = desc_of(name)
    rays = pinhole(name, 24, 16)
    planes, tab, col = composed(name, "pinhole", desc=d, rays=rays)
    ls = layers(tab, col, 4)
    n = len(rays)
    twins = {0: (1, (0.0, 1.0, 0.0)), 2: (3, (1.0, 1.0, 0.0)), 4: (5, (1.0, 0.0, 1.0))}
    seen = 0
    for l in range(3):
        for a, (b, rgb) in twins.items():
            m = (ls[l]["object"] == a) & (tab[b, :, 0] > 0)  # (the plane is wider than its triangle)
            seen += int(m.sum())
            assert (ls[l + 1]["object"][m] == b).all() and (ls[l + 1]["distance"][m] == ls[l]["distance"][m]).all()
            assert (ls[l + 1]["colour"][m] == np.array(rgb, np.float32)).all()
    assert seen >= 30
    r, s, cam = renderer(name)
    assert (r.accel_info().sph_nodes > 0) == (name == "ties_large")
    for rw in (24, 0):
        got = r.query_layers(rays, 4, raster_width=rw)
        for l in range(4):
            assert_planes(got[l], ls[l], (name, rw, "layer", l))
        w = closest_span(tab, col, lo=planes["distance"], after=np.full(n, INT32_MAX))
        both = (planes["object"] == 0) | (planes["object"] == 2)
        assert both.sum() >= 10 and not np.isin(w["object"][both], (0, 1, 2, 3)).any()
        assert_planes(hits(r, rays, lo=planes["distance"], after=np.full(n, INT32_MAX), raster_width=rw), w, (name, rw))
        # the any-hit's lower end is inclusive: with the winner left out its twin still occludes at lo = dist
        occ = shadow(r, rays, planes["object"], lo=planes["distance"], hi=planes["distance"], raster_width=rw)
        assert_occ(occ, any_hit_span(tab, planes["object"], lo=planes["distance"], hi=planes["distance"]), (name, rw))
        assert occ[both].all()
    r.close()


# ------------------------------------------------------------------ the 2^-20 band
@pytest.mark.parametrize("name,tri_accel", [("default", None), ("planes", None), ("stress4096", None), ("soup300", 1)])
def test_the_band(name, tri_accel):
    """From 1e6 behind, neighbouring distances differ by an ulp or not at all: layers 1 to 3, both sides of the upper
    end, and the segment up to the second distance with the winner left out."""
    rays, want, tab, col = ref(name, "far")
    r, s, cam = renderer(name, tri_accel)
    if tri_accel:
        assert r.accel_info().tri_nodes > 0
    ls = layers(tab, col, 3)
    got = r.query_layers(rays, 3)
    for l in range(3):
        assert_planes(got[l], ls[l], (name, "far layer", l))
    dist = want["distance"]
    assert_planes(hits(r, rays, hi=dist), want, (name, "far, hi = dist"))
    assert_planes(hits(r, rays, hi=below(dist)), closest_span(tab, col, hi=below(dist)), (name, "far, hi below"))
    d2 = second_distance(tab, col)
    w = any_hit_span(tab, want["object"], hi=d2)
    assert w.sum() >= 25
    assert_occ(shadow(r, rays, want["object"], hi=d2), w, (name, "far, skip winner, hi = second"))
    w = any_hit_span(tab, want["object"], hi=below(d2))
    assert_occ(shadow(r, rays, want["object"], hi=below(d2)), w, (name, "far, skip winner, hi below second"))
    r.close()


# ------------------------------------------------------------------ occlusion
@pytest.mark.parametrize("name", SCENES)
def test_segment_occlusion(name):
    """hi = the first distance occludes, one float below does not; with the winner left out the second distance
    decides; a lower end alone; Renderer.visible either side of the first crossing."""
    r, s, cam = renderer(name)
    for kind in ("pierce", "incoherent"):
        rays, want, tab, col = ref(name, kind)
        n = len(rays)
        dist, win = want["distance"], want["object"]
        hit = win >= 0
        occ = shadow(r, rays, hi=dist)
        assert_occ(occ, any_hit_span(tab, hi=dist), (name, kind, "hi = dist"))
        assert np.array_equal(occ, hit.astype(np.uint8))
        occ = shadow(r, rays, hi=below(dist), raster_width=21)
        assert_occ(occ, any_hit_span(tab, hi=below(dist)), (name, kind, "hi below dist"))
        assert not occ.any()
        d2 = second_distance(tab, col)
        for hi in (d2, below(d2)):
            assert_occ(shadow(r, rays, win, hi=hi, order="coherent"), any_hit_span(tab, win, hi=hi), (name, kind, "second"))
        for lo in (dist, above(dist)):
            assert_occ(shadow(r, rays, lo=lo, raster_width=24), any_hit_span(tab, lo=lo), (name, kind, "lo alone"))
            assert_occ(shadow(r, rays, lo=lo, hi=d2), any_hit_span(tab, lo=lo, hi=d2), (name, kind, "both ends"))
        if kind == "pierce":
            # b = origin + d s for s either side of the first crossing (t = dist / |d|, about)
            g = np.random.default_rng(20261023)
            o, d = rays[:, 0:3], rays[:, 3:6]
            t = dist.astype(np.float64) / np.linalg.norm(d.astype(np.float64), axis=1)
            sc = (t * np.where(np.arange(n) % 2 == 0, 0.5, 2.0) * g.uniform(0.9, 1.1, n)).astype(np.float32)
            b = (o + d * sc[:, None]).astype(np.float32)
            seg = (b - o).astype(np.float32)
            hi = np.sqrt(seg[:, 0] * seg[:, 0] + seg[:, 1] * seg[:, 1] + seg[:, 2] * seg[:, 2], dtype=np.float32)
            segrays = np.concatenate([o, seg], axis=1).astype(np.float32)
            from hits_helpers import table
            stab, _ = table(desc_of(name), segrays)
            w = 1 - any_hit_span(stab, hi=hi)
            assert w.sum() >= 100 and (w == 0).sum() >= 100
            vis = r.visible(o, b)
            assert vis.dtype == np.uint8 and np.array_equal(vis, w), (name, np.flatnonzero(vis != w)[:8].tolist())
            import torch
            with torch.cuda.stream(torch.cuda.Stream()):
                tv = r.visible(dev(o), dev(b))
                torch.cuda.current_stream().synchronize()
            assert np.array_equal(tv.cpu().numpy(), w)
            wskip = 1 - any_hit_span(stab, win, hi=hi)
            assert np.array_equal(r.visible(o, b, skip=win), wskip)
    r.close()


# ------------------------------------------------------------------ odd bounds
@pytest.mark.parametrize("name", ["default", "stress4096"])
def test_odd_bounds(name):
    """NaN, infinities, negative values and -0.0 as ends, and `after` outside [-1, objects), on one wave of rays: the
    definition's plain float comparisons decide."""
    rays, want, tab, col = ref(name, "pierce")
    rays, tab, col = rays[:64], tab[:, :64], col[:, :64]
    dist, win = want["distance"][:64], want["object"][:64]
    m = tab.shape[0]
    nan = np.float32(np.nan)
    r, s, cam = renderer(name)
    full = closest_span(tab, col)
    for lo, after, hi in ((nan, None, None), (None, None, nan), (INF, None, None), (-INF, None, None),
                          (None, None, INF), (None, None, -INF), (np.float32(-3.0), None, None),
                          (None, None, np.float32(-3.0)), (np.float32(-0.0), None, None), (None, None, np.float32(-0.0)),
                          (np.float32(0.0), None, np.float32(0.0)), (None, None, FLT_MAX), (FLT_MAX, None, None),
                          (dist, np.full(64, -5, np.int32), None), (dist, np.full(64, m, np.int32), None),
                          (dist, np.full(64, m + 1000, np.int32), None), (dist, np.full(64, -2 ** 31, np.int32), None),
                          (np.where(np.arange(64) % 2 == 0, nan, dist).astype(np.float32), win, np.where(np.arange(64) % 3 == 0, nan, INF).astype(np.float32))):
        f = lambda v, dt: None if v is None else np.broadcast_to(np.asarray(v, dt), (64,)).copy()
        lo_, af_, hi_ = f(lo, np.float32), f(after, np.int32), f(hi, np.float32)
        w = closest_span(tab, col, lo=lo_, after=af_, hi=hi_)
        assert_planes(hits(r, rays, lo=lo_, after=af_, hi=hi_), w, (name, "odd", str(lo)[:12], str(hi)[:12]))
        assert_occ(shadow(r, rays, lo=lo_, hi=hi_), any_hit_span(tab, lo=lo_, hi=hi_), (name, "odd any-hit"))
    for v in (nan, INF):
        assert (closest_span(tab, col, lo=v)["object"] == -1).all()
    assert (closest_span(tab, col, hi=np.float32(-3.0))["object"] == -1).all()
    assert_planes(closest_span(tab, col, lo=np.float32(-3.0), hi=FLT_MAX), full, "bounds nothing")
    r.close()


# ------------------------------------------------------------------ mechanics
@pytest.mark.parametrize("name", ["default", "stress4096"])
def test_sizes_splitting_and_orders(name):
    """Prefixes of 1, 63, 64 and 65 rays; launch limits of one wave and one tile row; the ordered forms with the
    coherent permutation and its reverse, the span arrays staying in ray order."""
    rays, want, tab, col = ref(name, "pierce")
    n = len(rays)
    g = np.random.default_rng(20261024)
    dist = want["distance"]
    lo = np.where(np.arange(n) % 2 == 0, dist, np.float32(-1.0)).astype(np.float32)
    after = np.where(np.arange(n) % 4 == 0, want["object"], -1).astype(np.int32)
    hi = (dist.astype(np.float64) * 10.0 ** g.uniform(-0.3, 1.0, n)).astype(np.float32)
    w = closest_span(tab, col, lo=lo, after=after, hi=hi)
    assert (w["object"] >= 0).sum() >= 50 and (w["object"] != want["object"]).sum() >= 50
    wo = any_hit_span(tab, want["object"], lo=lo, hi=hi)
    r, s, cam = renderer(name)
    for k in (1, 63, 64, 65):
        for rw in (0, 8):
            assert_planes(hits(r, rays[:k], lo=lo[:k], after=after[:k], hi=hi[:k], raster_width=rw),
                          {p: v[:k] for p, v in w.items()}, (name, k, rw))
            assert_occ(shadow(r, rays[:k], want["object"][:k], lo=lo[:k], hi=hi[:k], raster_width=rw), wo[:k], (name, k, rw))
    order = r.order_rays(rays)
    assert sorted(order.tolist()) == list(range(n))
    for limit, rws in ((None, (0,)), (64, (0,)), (1, (0, 8, 24))):  # None: the default limit, one launch
        if limit:
            r.set_launch_traces(limit)
        for rw in rws:
            assert_planes(hits(r, rays, lo=lo, after=after, hi=hi, raster_width=rw), w, (name, "split", limit, rw))
            assert_occ(shadow(r, rays, want["object"], lo=lo, hi=hi, raster_width=rw), wo, (name, "split", limit, rw))
        for o in (order, order[::-1].copy()):
            assert_planes(hits(r, rays, lo=lo, after=after, hi=hi, order=o), w, (name, "ordered", limit))
            assert_occ(shadow(r, rays, want["object"], lo=lo, hi=hi, order=o), wo, (name, "ordered", limit))
            assert_planes(r.query_hits(rays, lo=lo, after=after, hi=hi, order=o), w, (name, "ordered, numpy", limit))
            assert_occ(r.occluded(rays, want["object"], lo=lo, hi=hi, order=o), wo, (name, "ordered, numpy", limit))
    # the host forms
    r.set_launch_traces(128)
    for rw in (0, 21):
        assert_planes(r.query_hits(rays, lo=lo, after=after, hi=hi, raster_width=rw), w, (name, "host", rw))
        assert_occ(r.occluded(rays, want["object"], lo=lo, hi=hi, raster_width=rw), wo, (name, "host", rw))
    assert_planes(r.query_hits(rays, hi=hi, want=("distance", "normal")),
                  {p: closest_span(tab, col, hi=hi)[p] for p in ("distance", "normal")}, (name, "host, hi alone"))
    r.close()


@pytest.mark.parametrize("name", ["default", "planes300"])
def test_host_forms_equal_the_device_forms_across_a_launch_split(name):
    """Through numpy (the host forms) and through a tensor (the device forms) every word is the same, for each plane
    asked alone and all six, without ends and with hi alone, and for the any-hit with and without skip -- on the
    smallest batches that take two launches: 65 rays at a limit of 64 (the second launch one ray), and a 21-wide raster
    of 189 rays at a limit of 168 (one tile row of 8 x 21, then one row)."""
    r, s, cam = renderer(name)
    for n, limit, rw in ((65, 64, 0), (189, 168, 21)):
        rays = pierce_rays(name)[:n]
        r.set_launch_traces(limit)
        full = hits(r, rays, raster_width=rw)
        assert (full["object"] >= 0).sum() >= n // 2 and full["object"][-1] >= 0  # (the planes are not all misses)
        with np.errstate(over="ignore"):  # (a miss's FLT_MAX doubled is +inf)
            hi = (full["distance"] * np.where(np.arange(n) % 2 == 0, 2.0, 0.5).astype(np.float32)).astype(np.float32)
        for ends in ({}, {"hi": hi}):
            tag = (name, n, rw, tuple(ends))
            for want in [(k,) for k in PLANES] + [PLANES]:
                dev_out = hits(r, rays, raster_width=rw, want=want, **ends)
                host_out = r.query_hits(rays, raster_width=rw, want=want, **ends)
                assert tuple(host_out) == want and tuple(dev_out) == want, tag
                assert all(isinstance(v, np.ndarray) for v in host_out.values()), tag
                assert_planes(host_out, dev_out, tag + (want,))
                if not ends:
                    assert_planes(dev_out, {k: full[k] for k in want}, tag + (want, "alone = among six"))
            for skip in (None, full["object"]):
                assert_occ(r.occluded(rays, skip, raster_width=rw, **ends), shadow(r, rays, skip, raster_width=rw, **ends),
                           tag + ("any-hit", skip is not None))
        cut = hits(r, rays, raster_width=rw, hi=hi)["object"]
        assert (cut != full["object"]).sum() >= n // 8  # (hi does cut winners off)
    r.close()


def test_sentinels_and_unrequested_planes():
    """16 sentinel words either side of every output and span buffer stay as they were; an unrequested plane stays
    wholly as it was."""
    import torch
    L = _lib.load()
    name = "planes300"
    rays, want, tab, col = ref(name, "pierce")
    n = len(rays)
    dist = want["distance"]
    lo, after, hi = dist.copy(), want["object"].copy(), above(second_distance(tab, col))
    w = closest_span(tab, col, lo=lo, after=after, hi=hi)
    wo = any_hit_span(tab, want["object"], lo=lo, hi=hi)
    r, s, cam = renderer(name)
    d_rays = dev(rays)
    SENT, PAD = 0x5A5A5A5A, 16
    words = {k: n * (1 if k in ("object", "distance") else 3) for k in PLANES}

    def padded(a):
        t = torch.full((PAD + a.size + PAD,), SENT, dtype=torch.int32, device="cuda")
        t[PAD:PAD + a.size] = torch.from_numpy(a.view(np.int32).copy()).cuda()
        return t

    for off, asked in ((0, PLANES), (1, PLANES), (0, ("object", "normal")), (1, ("distance", "colour"))):
        buf = {k: torch.full((PAD + off + words[k] + PAD,), SENT, dtype=torch.int32, device="cuda") for k in PLANES}
        ends = {"d_lo": padded(lo), "d_after": padded(after), "d_hi": padded(hi)}
        occ = torch.full((PAD + n + PAD,), 0x5A, dtype=torch.uint8, device="cuda")
        d_skip = padded(want["object"])
        torch.cuda.synchronize()  # the renderer's own stream is not ordered with torch's
        hp = _lib.HitPlanes()
        for k in asked:
            setattr(hp, k, buf[k].data_ptr() + 4 * (PAD + off))
        sp = _lib.RaySpan(**{k: t.data_ptr() + 4 * PAD for k, t in ends.items()})
        _lib.check(L.rfx_query_hits_span(r._h, C.c_void_p(d_rays.data_ptr()), C.byref(sp), n, 24 if off else 0,
                                         C.byref(hp), None))
        _lib.check(L.rfx_query_occluded_span(r._h, C.c_void_p(d_rays.data_ptr()), C.c_void_p(d_skip.data_ptr() + 4 * PAD),
                                             C.byref(sp), n, 24 if off else 0, C.c_void_p(occ.data_ptr() + PAD), None))
        r.synchronize()
        for k in PLANES:
            b = buf[k].cpu().numpy()
            if k not in asked:
                assert (b == SENT).all(), (k, off, asked)
                continue
            assert (b[:PAD + off] == SENT).all() and (b[PAD + off + words[k]:] == SENT).all(), (k, off)
            got = b[PAD + off:PAD + off + words[k]].view(w[k].dtype).reshape(w[k].shape)
            assert same_bits(got, w[k]).size == 0, (k, off, asked)
        for k, a in (("d_lo", lo), ("d_after", after), ("d_hi", hi)):
            b = ends[k].cpu().numpy()
            assert (b[:PAD] == SENT).all() and (b[PAD + n:] == SENT).all() and (b[PAD:PAD + n] == a.view(np.int32)).all(), k
        o = occ.cpu().numpy()
        assert (o[:PAD] == 0x5A).all() and (o[PAD + n:] == 0x5A).all()
        assert_occ(o[PAD:PAD + n].copy(), wo, ("sentinels", off))
    r.close()


def test_span_queries_leave_the_renderer_state_alone():
    """The random streams read the same before and after; a frame rendered after span queries is the golden frame, and
    so is the still view's second frame with span queries in between; a rewind after "frame, then query" succeeds."""
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
    rays, want, tab, col = ref("default", "pierce")
    l2 = layers(tab, col, 2)[1]
    R = Render(sphere_seed=c["sphere_seed"], jitter_seed=0, load_default_scene=False)
    R.scene, R.camera = build_scene(scene("default"))
    R.setImageSize(W, H)
    r = R._r
    r.set_scene(R.scene)

    def frame():
        R.renderBegin(depth, 1, False)
        while R.renderNext(W * H):
            pass

    def queries(tag):
        assert_planes(hits(r, rays, lo=want["distance"], after=want["object"]), l2, tag)
        assert_occ(shadow(r, rays, hi=want["distance"]), any_hit_span(tab, hi=want["distance"]), tag)
        assert_planes(hits(r, rays, hi=want["distance"], order="coherent"), want, tag)

    queries("before")
    assert r.get_rng() == (c["sphere_seed"], 0)
    frame()
    R.synchronize()
    assert R.image.tobytes() == g["rgb"].tobytes()
    assert r.get_rng() == (seed1, 0)
    queries("between")
    assert r.get_rng() == (seed1, 0)
    frame()
    R.synchronize()
    assert R.image.tobytes() == o.image.tobytes()
    assert r.get_rng() == (o.sphere_seed.value, 0)
    assert_planes(r.query_hits(rays, lo=want["distance"], after=want["object"]), l2, "host form")
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
    order = torch.arange(64, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    p = lambda t: C.c_void_p(t.data_ptr())
    hp, none, sp = _lib.HitPlanes(object=obj.data_ptr()), _lib.HitPlanes(), _lib.RaySpan()
    bare = Renderer(sphere_seed=SEED)
    assert L.rfx_query_hits_span(bare._h, p(rays), C.byref(sp), 64, 0, C.byref(hp), None) == RFX_ERR_STATE  # no scene
    assert L.rfx_query_occluded_span(bare._h, p(rays), None, C.byref(sp), 64, 0, p(occ), None) == RFX_ERR_STATE
    assert L.rfx_query_hits_span_ordered(bare._h, p(rays), None, p(order), 64, C.byref(hp), None) == RFX_ERR_STATE
    bare.close()
    r, s, cam = renderer("default")
    assert L.rfx_query_hits_span(r._h, p(rays), C.byref(sp), 0, 0, C.byref(hp), None) == RFX_ERR_ARG
    assert L.rfx_query_hits_span(r._h, None, C.byref(sp), 64, 0, C.byref(hp), None) == RFX_ERR_ARG
    assert L.rfx_query_hits_span(r._h, p(rays), C.byref(sp), 64, 0, None, None) == RFX_ERR_ARG
    assert L.rfx_query_hits_span(r._h, p(rays), C.byref(sp), 64, 0, C.byref(none), None) == RFX_ERR_ARG
    assert L.rfx_query_occluded_span(r._h, p(rays), None, C.byref(sp), 0, 0, p(occ), None) == RFX_ERR_ARG
    assert L.rfx_query_occluded_span(r._h, None, None, C.byref(sp), 64, 0, p(occ), None) == RFX_ERR_ARG
    assert L.rfx_query_occluded_span(r._h, p(rays), None, C.byref(sp), 64, 0, None, None) == RFX_ERR_ARG
    assert L.rfx_query_hits_span_ordered(r._h, p(rays), C.byref(sp), None, 64, C.byref(hp), None) == RFX_ERR_ARG
    assert L.rfx_query_hits_span_ordered(r._h, p(rays), C.byref(sp), p(order), 2 ** 32, C.byref(hp), None) == RFX_ERR_ARG
    assert L.rfx_query_occluded_span_ordered(r._h, p(rays), None, C.byref(sp), None, 64, p(occ), None) == RFX_ERR_ARG
    host = np.zeros(64, np.uint8)
    assert L.rfx_query_hits_span_host(r._h, None, C.byref(sp), 64, 0, C.byref(hp)) == RFX_ERR_ARG
    assert L.rfx_query_occluded_span_host(r._h, None, None, C.byref(sp), 64, 0,
                                          host.ctypes.data_as(C.POINTER(C.c_uint8))) == RFX_ERR_ARG
    assert L.rfx_query_hits_span(r._h, p(rays), None, 64, 0, C.byref(hp), None) == 0
    r.synchronize()
    with pytest.raises(ValueError):
        r.query_hits(rays, after=obj)  # after goes with lo
    with pytest.raises(ValueError):
        r.query_hits(rays, hi=torch.zeros(63, device="cuda"))
    with pytest.raises(ValueError):
        r.query_layers(rays, 0)
    r.close()


def test_render_pick_layers():
    """Render.pick(x, y, layer) under a few pixels of the default scene at 160 x 120: what lies behind `layer` hits of
    that pixel's pinhole ray, (-1, FLT_MAX) once the ray has run out."""
    from reflaxman_amd.render import Render, build_scene
    d = scene("default")
    W, H = 160, 120
    eye, at, fov = d.camera
    view = orc.camera_view(eye, at)
    frame = cameras.pinhole_rays(eye, view, fov, W, H)
    planes, tab, col = composed("default", "pinhole160", desc=d, rays=frame)
    ls = layers(tab, col, 4)
    c = counts(tab).reshape(H, W)
    mid = lambda mask: tuple(int(v) for v in np.argwhere(mask)[len(np.argwhere(mask)) // 2][::-1])
    assert (c >= 2).any() and (c == 1).any() and (c == 0).any()
    one = mid(c == 1)
    picks = [mid(c == k) for k in range(int(c.max()) + 1) if (c == k).any()] + [(0, 0), (W - 1, H - 1)]
    R = Render(sphere_seed=SEED, jitter_seed=77, load_default_scene=False)
    R.scene, R.camera = build_scene(d)
    R.setImageSize(W, H)
    for (x, y) in picks:
        i = y * W + x
        assert R.pick(x, y) == R.pick(x, y, 0)
        for l in range(4):
            o, dist = R.pick(x, y, layer=l)
            assert o == int(ls[l]["object"][i]), (x, y, l)
            assert np.float32(dist).tobytes() == ls[l]["distance"][i].tobytes(), (x, y, l)
    x, y = one
    assert R.pick(x, y, 1) == (-1, float(FLT_MAX)) and R.pick(x, y, 3) == (-1, float(FLT_MAX))
    with pytest.raises(ValueError):
        R.pick(0, 0, layer=-1)
    assert R.getRng() == (SEED, 77)
    R.close()
