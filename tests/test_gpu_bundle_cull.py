"""The wave-bundle culls on the device, on the bundles that stress them (tests/test_bundle_cull_bound.py is their CPU
replay): waves of 64 coherent rays next to the silhouettes of skewed, sliver and tiny triangles, grazing and leaving
their planes, through the hit queries, the ray-batch trace, the paths, the per-view primary masks and whole frames,
each against the reference's own answer bit for bit.

Two descriptions with fixed seeds: `small` -- 24 triangles of test_tri_box_bound's recipe, at least 4 in each cond class
[3, 100), [100, 300), >= 300, and 8 spheres, so cull_small with its plane rule and the footprint -- with 1, 3 and 6
lights (the one-light and far-light cfgs, several lights, more than kPrimLights), some wide enough to cross
make_bundle_ball's sb < 0.5; `large` -- 40 spheres and the same triangles (cull_chunk), with and without a triangle tree.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np
import pytest

import bundle_cull as bc
import oracle as orc
import paths_helpers as ph
from bundle_cull import F
from hits_helpers import PLANES, any_hit, compose, same_bits, table
from rays_helpers import oracle_trace
from reflaxman_amd import cameras, scenes

pytestmark = pytest.mark.gpu

SEED = 97531
JITTER = 99
NB = 192                     # crafted bundles: 64 consecutive rays each
NARROW_COS = 0.9995          # rfx_config.h RFX_NARROW_BUNDLE_COS
K_VERY_SMALL = F(1.0842021724855044e-19)
LIGHTS = {1: "small1", 3: "small3", 6: "small6"}
W, H = 64, 40


# ------------------------------------------------------------------------------------------ the two descriptions
@functools.lru_cache(maxsize=None)
def geometry():
    """(the 24 triangles' geometry, sphere centres (48, 3) and radii): the first 8 spheres are the small scene's"""
    G = bc.triangles(512, 20261023)
    cls = bc.cond_class(G.cond)
    pick = np.concatenate([np.flatnonzero(cls == k)[:8] for k in range(3)])
    pick = pick[np.random.default_rng(3).permutation(len(pick))]
    # the scene is drawn together: a triangle's v0 moved to within +-8 of the origin keeps its shape
    V = G.V[pick] - G.V[pick][:, :1] + np.random.default_rng(4).uniform(-8.0, 8.0, (24, 1, 3))
    G = bc.geometry(V.astype(F).astype(np.float64))
    assert all((bc.cond_class(G.cond) == k).sum() >= 4 for k in range(3)), G.cond
    rng = np.random.default_rng(5)
    c = rng.uniform(-10.0, 10.0, (48, 3)).astype(F).astype(np.float64)
    r = np.exp(rng.uniform(np.log(0.05), np.log(3.0), 48)).astype(F).astype(np.float64)
    return G, c, r


@functools.lru_cache(maxsize=None)
def desc_of(key):
    G, c, r = geometry()
    nl = {"small1": 1, "small3": 3, "small6": 6, "large": 3}[key]
    d = scenes.SceneDesc("cull_" + key, (0.9, 0.9, 1.0, 0.1), ((0.0, 10.0, -30.0), (0.0, 0.0, 0.0), 1.0))
    rng = np.random.default_rng(6)
    for q in range(6):   # every other light wide: R / |d| passes 0.5 for the hits within two radii of it
        o = rng.uniform(-1.0, 1.0, 3) * (20.0, 8.0, 20.0) + (0.0, 22.0, 0.0)
        rad, col = (12.0, 0.6)[q % 2], rng.uniform(0.4, 1.0, 3)
        if q < nl:
            d.add_light(o, rad, col, 0.9 / nl)
    mats = [(scenes.METAL, 0.5), (scenes.DIELECTRIC, 0.3), (scenes.METAL, 0.8)]
    ns = 40 if key == "large" else 8
    for i in range(max(ns, 24)):   # spheres and triangles interleaved in insertion order
        if i < ns:
            m = mats[i % 3]
            d.add_sphere(c[i], r[i], m[0], rng.uniform(0.2, 1.0, 3), m[1])
        if i < 24:
            m = mats[(i + 1) % 3]
            d.add_triangle(*G.V[i], m[0], rng.uniform(0.2, 1.0, 3), m[1])
    return d


def object_index(desc):
    """(object indices of the spheres, of the triangles) in insertion order"""
    return ([j for j, ob in enumerate(desc.objects) if ob[0] == "sphere"],
            [j for j, ob in enumerate(desc.objects) if ob[0] == "triangle"])


def renderer(key, tri_accel=None):
    from reflaxman_amd.render import Renderer, build_scene
    s, cam = build_scene(desc_of(key))
    r = Renderer(sphere_seed=SEED, jitter_seed=JITTER)
    if tri_accel is not None:
        r.set_tri_accel(tri_accel)
    r.set_scene(s)
    r._keep = (s, cam)
    return r


# ------------------------------------------------------------------------------------------ crafted bundles
@functools.lru_cache(maxsize=None)
def crafted():
    """192 bundles of 64 rays, each aimed at a real object of the descriptions (the 24 triangles, the first 8
    spheres): 48 aimed at triangles, 32 at spheres, 48 departing, 32 + 32 of either with spread origins, the families
    interleaved.  (n, 6) float32 records, bundle b = rays 64 b .. 64 b + 63."""
    G, c, r = geometry()
    sub = lambda idx: bc.geometry(G.V[idx])
    tri = lambda n, k: (np.arange(n) * 5 + k) % 24
    parts = []
    g = sub(tri(48, 0))
    p, out = bc.tri_silhouette(g, 11)
    parts.append(bc.aimed(p, out, g.nrm, g.size, 12))
    si = np.arange(32) % 8
    parts.append(bc.aimed_sphere(c[si], r[si], 13))
    parts.append(bc.departing(sub(tri(48, 1)), 14))
    g = sub(tri(32, 2))
    p, out = bc.tri_silhouette(g, 15)
    parts.append(bc.aimed(p, out, g.nrm, g.size, 16, spread=True))
    parts.append(bc.departing(sub(tri(32, 3)), 17, spread=True))
    o, d = (np.concatenate([q[k] for q in parts]) for k in (0, 1))
    assert len(o) == NB
    perm = np.random.default_rng(18).permutation(NB)
    rays = np.concatenate([o[perm], d[perm]], axis=2).reshape(-1, 6)
    assert np.isfinite(rays).all() and not (rays[:, 3:6] == 0).any()
    rays.setflags(write=False)
    return rays


def composed(key):
    return compose(desc_of(key), crafted(), key=("crafted", key))


def replay_small(rays, live=None):
    """tests/bundle_cull.py on the waves of a ray batch against the small description's own records: (B, keep (n, 64),
    valid lanes (64,) bool)"""
    from reflaxman_amd.render import build_scene
    s, _ = build_scene(desc_of("small1"))
    recs, tris, valid = s.cull_dump()
    n = len(rays) // 64
    o, d = rays[:n * 64, 0:3].reshape(n, 64, 3), rays[:n * 64, 3:6].reshape(n, 64, 3)
    rng = np.random.default_rng(1)
    B = bc.make_bundle(o, d, np.ones((n, 64), bool) if live is None else live, rng)
    keep = bc.cull_small(recs, tris, valid, B, rng)
    vb = np.array([(valid >> l) & 1 for l in range(64)], bool)
    return B, keep, vb


def test_crafted_bundles_are_culled_in_the_replay():
    """non-vacuity of the batches below: the bound is usable for >= 3/4 of the bundles, drops an object in >= 1/2, and
    the cones lie on both sides of RFX_NARROW_BUNDLE_COS"""
    B, keep, vb = replay_small(crafted())
    assert B.ok.mean() >= 0.75
    dropped = (~keep & vb[None, :]).any(1) & B.ok
    print(f"crafted: B.ok {B.ok.mean():.3f}, drops an object {dropped.mean():.3f}, mean kept "
          f"{keep[B.ok].sum(1).mean():.1f} of {int(vb.sum())}, narrow {np.mean(B.cosa > NARROW_COS):.3f}")
    assert dropped.mean() >= 0.5
    assert (B.cosa[B.ok] > NARROW_COS).sum() >= NB // 8 and (B.cosa[B.ok] < NARROW_COS).sum() >= NB // 8
    want, tab = composed("small1")
    assert (want["object"] >= 0).mean() > 0.05


@pytest.mark.parametrize("key,tri_accel", [("small1", None), ("large", 0), ("large", 1)])
def test_crafted_bundles_through_the_queries(key, tri_accel):
    """query_hits (all six planes) and occluded (nothing skipped; the winner skipped) equal the composed reference bit
    for bit: as a linear batch (a wave is 64 consecutive rays), as a raster 8 wide (a tile is the same 64) and as a linear
    batch in the coherent order, and with the last wave 27 rays short"""
    from test_gpu_hits import assert_planes, hits, shadow
    rays = crafted()
    want, tab = composed(key)
    r = renderer(key, tri_accel)
    if key == "large":
        assert (r.accel_info().tri_nodes > 0) == bool(tri_accel)
    for n in (len(rays), len(rays) - 27):
        w = {k: v[:n] for k, v in want.items()}
        for rw, order in ((0, None), (8, None), (0, "coherent")):   # (an order goes with a linear batch)
            tag = (key, tri_accel, n, rw, order)
            got = hits(r, rays[:n], raster_width=rw, order=order)
            assert sorted(got) == sorted(PLANES)
            assert_planes(got, w, tag)
            occ = shadow(r, rays[:n], raster_width=rw, order=order)
            assert np.array_equal(occ, any_hit(tab)[:n]), tag
            own = shadow(r, rays[:n], w["object"], raster_width=rw, order=order)
            assert np.array_equal(own, any_hit(tab, want["object"])[:n]), tag
    r.close()


@functools.lru_cache(maxsize=None)
def traced(key):
    rgb, _ = oracle_trace(desc_of(key), crafted()[:2048], 3, SEED)
    rgb.setflags(write=False)
    return rgb


@pytest.mark.parametrize("key,tri_accel", [("small1", None), ("small3", None), ("small6", None), ("large", 0), ("large", 1)])
def test_crafted_bundles_through_the_trace_and_the_paths(key, tri_accel):
    """the first 32 bundles at depth 3 -- the bounce loop's secondary and shadow bundles (make_bundle, make_bundle_far)
    start on these triangles -- through rfx_trace_rays and through the paths stepped to 3"""
    from test_gpu_rays import trace
    rays = np.array(crafted()[:2048])
    want = traced(key)
    r = renderer(key, tri_accel)
    got = trace(r, rays, 3)
    bad = same_bits(got, want)
    assert bad.size == 0, (key, "trace", int(bad.size), bad[:8].tolist(), got[bad[:2]].tolist(), want[bad[:2]].tolist())
    st = ph.State(rays)
    r.set_rng(SEED, JITTER)
    assert ph.begin(r, st) == 0
    assert ph.step(r, st, 3) == 0
    bad = same_bits(st.get("colour"), want)
    assert bad.size == 0, (key, "paths", int(bad.size), bad[:8].tolist())
    assert np.array_equal(st.get("argb"), orc.argb_of(want))
    r.close()


# ------------------------------------------------------------------------------------------ views
@functools.lru_cache(maxsize=None)
def views():
    """12 cameras (eye, at, fov) on the small description"""
    G, c, r = geometry()
    v = []
    for k in range(5):   # generic orbit positions
        a = 0.4 + 1.25 * k
        v.append(((28.0 * np.cos(a), 6.0 * (k - 1.5), 28.0 * np.sin(a)), (1.0 * k, 0.5, -1.0), 1.0))
    lo = int(np.argmax(np.where(G.cond < 100.0, G.size, 0.0)))   # the largest well-conditioned triangle
    n, cen, rad = G.nrm[lo], G.cen[lo], G.rad[lo]
    t = bc._unit(G.V[lo, 1] - G.V[lo, 0])
    for sgn in (1.0, -1.0):   # 1e-3 sizes over a triangle's plane, looking along it; the same from below
        up = n * (sgn * 1e-3 * G.size[lo])
        v.append((tuple(cen - t * 1.5 * rad + up), tuple(cen + up), 1.0))
    v.append((tuple(c[2] + 0.3 * r[2] * np.array([0.3, 0.5, -0.8])), (0.0, 0.0, 0.0), 1.0))   # inside a sphere
    big = int(np.argmax(G.rad))
    v.append((tuple(G.cen[big] + G.nrm[big] * 0.3 * G.rad[big]), tuple(G.cen[big] + t * G.rad[big]), 1.0))  # inside a triangle's bounding sphere
    edge = 0.5 * (G.V[lo, 0] + G.V[lo, 1])
    v.append((tuple(edge + bc._unit(np.array([0.3, 0.5, -0.8])) * 1e3), tuple(edge), 1e-3))   # fov 1e-3 from 1e3 away
    v.append(((20.0, 8.0, -30.0), (0.0, 0.0, 0.0), 2.5))                                       # fov 2.5
    v.append(((0.0, 10.0, -30.0), (0.0, 20.0, -60.0), 1.0))                                   # straight away
    assert len(v) == 12
    return tuple((tuple(float(x) for x in e), tuple(float(x) for x in a), float(f)) for e, a, f in v)


def view_desc(key, vi):
    return dataclasses.replace(desc_of(key), camera=views()[vi])


def view_rays(vi):
    eye, at, fov = views()[vi]
    return cameras.pinhole_rays(eye, orc.camera_view(eye, at), fov, W, H)


@functools.lru_cache(maxsize=None)
def view_table(vi):
    """the composed reference of a view's 64 x 40 primary rays (the objects are the same in every small variant)"""
    want, tab = compose(desc_of("small1"), view_rays(vi), key=("view", vi))
    return want, tab


def bit_of(desc):
    """mask bit of each object index (rfx_queries.h: sphere i in lane (i & 1) 16 + (i >> 1), triangle i in 32 + i)"""
    sph, tri = object_index(desc)
    bit = np.full(len(desc.objects), -1)
    for i, j in enumerate(sph):
        bit[j] = (i & 1) * 16 + (i >> 1)
    for i, j in enumerate(tri):
        bit[j] = 32 + i
    return bit


def bits(objs, bit):
    m = 0
    for j in objs:
        m |= 1 << int(bit[j])
    return m


@functools.lru_cache(maxsize=None)
def conservative_masks(nl, vi):
    from test_gpu_prim_exact import Rig
    g = Rig(view_desc(LIGHTS[nl], vi), W, H, 2, 0, jitter_seed=JITTER)
    g.frame(1)
    m = g.masks().copy()
    g.close()
    m.setflags(write=False)
    return m


@pytest.mark.parametrize("vi", range(12))
def test_primary_word_holds_every_reported_object(vi):
    """set_prim_masks(2), set_prim_exact(0), one sample: word 0 of every tile holds the bit of every object the oracle
    table reports for any of the tile's pixels"""
    from test_gpu_prim_exact import tiles_of
    desc = desc_of("small1")
    bit = bit_of(desc)
    want, tab = view_table(vi)
    rep = ((tab[:, :, 0] > 0) | (tab[:, :, 14] > 0)).reshape(len(desc.objects), H, W)
    m = conservative_masks(1, vi)
    for ty, tx, _ in tiles_of(rep[0], H, W):
        need = bits(np.flatnonzero(rep[:, 8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8].any((1, 2))), bit)
        got = int(m[ty, tx, 0])
        assert got & need == need, (vi, ty, tx, hex(got), hex(need))


def test_primary_words_drop_objects_and_the_footprint_decides():
    """non-vacuity over the 12 views: word 0 drops >= 1/4 of the valid bits summed over the tiles, and the footprint
    decides a tile (the replay with and without it differs) in >= 6 views"""
    from reflaxman_amd.render import build_scene
    s, _ = build_scene(desc_of("small1"))
    recs, tris, valid = s.cull_dump()
    nvalid = bin(valid).count("1")
    kept = total = foot_views = 0
    for vi in range(12):
        m = conservative_masks(1, vi)[:, :W // 8, 0]
        kept += sum(bin(int(x)).count("1") for x in m.reshape(-1))
        total += nvalid * m.size
        rays = view_rays(vi).reshape(H // 8, 8, W // 8, 8, 6).transpose(0, 2, 1, 3, 4).reshape(-1, 64, 6)
        rng = np.random.default_rng(2)
        B = bc.make_bundle(rays[:, :, 0:3], rays[:, :, 3:6], np.ones(rays.shape[:2], bool), rng)
        a = bc.cull_small(recs, tris, valid, B, np.random.default_rng(3), foot=False)
        b = bc.cull_small(recs, tris, valid, B, np.random.default_rng(3), foot=True)
        foot_views += bool((a != b).any())
    print(f"word 0 keeps {kept} of {total} valid bits; the footprint decides in {foot_views} of 12 views")
    assert kept <= 0.75 * total
    assert foot_views >= 6


@pytest.mark.parametrize("nl", [1, 3, 6])
@pytest.mark.parametrize("vi", range(12))
def test_shadow_words_hold_every_reported_occluder(nl, vi):
    """word 1 + q (q < 4): for each pixel whose composed winner faces light q (dot(dtl, norm) > kVerySmall, Scene.cpp:125;
    within 1e-6 of it: unsure, skipped) the shadow rays from the oracle's point toward the light for 16 sampled randDir
    (Scene.cpp:128-129 in float32); the word holds every object the oracle reports for any of them, but the one the
    pixel's own hit lies on"""
    from test_gpu_prim_exact import tiles_of
    desc = desc_of(LIGHTS[nl])
    bit = bit_of(desc)
    want, _ = view_table(vi)
    m = conservative_masks(nl, vi)
    hit = want["object"] >= 0
    rd = bc.ball_samples()
    skipped = lit = 0
    for q in range(min(nl, 4)):
        lo, lr = np.asarray(desc.lights[q][0], F), F(desc.lights[q][1])
        dtl = lo[None, :] - want["point"]
        nrm = want["normal"]
        dot = dtl[:, 0] * nrm[:, 0] + dtl[:, 1] * nrm[:, 1] + dtl[:, 2] * nrm[:, 2]
        unsure = hit & (np.abs(dot - K_VERY_SMALL) < F(1e-6))
        facing = hit & (dot > K_VERY_SMALL) & ~unsure
        skipped, lit = skipped + int(unsure.sum()), lit + int(facing.sum())
        idx = np.flatnonzero(facing)
        need = np.zeros((len(desc.objects), H * W), bool)
        if idx.size:
            d = bc.shadow_rays(want["point"][idx][:, None, :], dtl[idx][:, None, :], np.full(idx.size, lr), rd)[:, 0]
            o = np.broadcast_to(want["point"][idx][:, None, :], d.shape)
            tab, _ = table(desc, np.concatenate([o, d], axis=2).reshape(-1, 6))
            rep = ((tab[:, :, 0] > 0) | (tab[:, :, 14] > 0)).reshape(len(desc.objects), idx.size, len(rd)).any(2)
            rep[want["object"][idx], np.arange(idx.size)] = False
            need[:, idx] = rep
        need = need.reshape(len(desc.objects), H, W)
        for ty, tx, _ in tiles_of(need[0], H, W):
            nb = bits(np.flatnonzero(need[:, 8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8].any((1, 2))), bit)
            got = int(m[ty, tx, 1 + q])
            assert got & nb == nb, (nl, vi, q, ty, tx, hex(got), hex(nb))
    assert skipped <= 0.02 * max(1, min(nl, 4)) * H * W, (skipped, lit)


# ------------------------------------------------------------------------------------------ frames
def gpu_frames(desc, depth, ss, additive, frames, masks, exact):
    from reflaxman_amd.render import Render, build_scene
    r = Render(device=0, sphere_seed=SEED, jitter_seed=JITTER, load_default_scene=False)
    r.scene, r.camera = build_scene(desc)
    r.setImageSize(W, H)
    r._r.set_prim_masks(masks)
    if exact is not None:
        r._r.set_prim_exact(exact)
    out = []
    for _ in range(frames):
        r.renderBegin(depth, ss, additive)
        while r.renderNext(W * H):
            pass
        r.synchronize()
        out.append((r.imagePixels().tobytes(), r.copyImage().tobytes()))
    r.close()
    return out


def oracle_frames(desc, depth, ss, additive, frames):
    o = orc.OracleRender(desc, SEED, JITTER)
    o.set_image_size(W, H)
    out = []
    for _ in range(frames):
        o.render(depth, ss, additive)
        out.append((o.image_pixels().tobytes(), o.argb().tobytes()))
    return out


# (ss, additive, frames, (masks mode, exact) runs): the last is the still view rendered twice under masks mode 1
ALL_MODES = ((0, None), (2, 0), (2, 1))
FORMS = [(1, False, 1, ALL_MODES), (2, False, 1, ALL_MODES), (4, False, 1, ALL_MODES), (1, True, 3, ALL_MODES),
         (1, False, 2, ((1, None),))]


@pytest.mark.parametrize("nl", [1, 3, 6])
@pytest.mark.parametrize("vi", range(12))
def test_frames_under_the_views(nl, vi):
    """64 x 40 at depth 6 against the oracle with the view's camera, f32 and ARGB8 bit for bit, without masks, with the
    conservative masks and with the exact ones: ss 1, ss 2, ss 4, ss 1 additive over 3 frames, and the still view
    rendered twice under masks mode 1 (built when the view repeats)"""
    desc = view_desc(LIGHTS[nl], vi)
    for ss, additive, frames, modes in FORMS:
        want = oracle_frames(desc, 6, ss, additive, frames)
        for masks, exact in modes:
            got = gpu_frames(desc, 6, ss, additive, frames, masks, exact)
            assert got == want, (nl, vi, ss, additive, frames, masks, exact,
                                 [int(np.sum(np.frombuffer(g[0], np.uint32) != np.frombuffer(w[0], np.uint32)))
                                  for g, w in zip(got, want)])


@pytest.mark.parametrize("tri_accel", [0, 1])
def test_large_description_frame(tri_accel):
    """the large description (cull_chunk; with and without the triangle tree) at depth 6, one sample"""
    from reflaxman_amd.render import Render, build_scene
    desc = desc_of("large")
    want = oracle_frames(desc, 6, 1, False, 1)
    r = Render(device=0, sphere_seed=SEED, jitter_seed=JITTER, load_default_scene=False)
    r._r.set_tri_accel(tri_accel)
    r.scene, r.camera = build_scene(desc)
    r.setImageSize(W, H)
    r.renderBegin(6, 1, False)
    while r.renderNext(W * H):
        pass
    r.synchronize()
    got = [(r.imagePixels().tobytes(), r.copyImage().tobytes())]
    r.close()
    assert got == want
