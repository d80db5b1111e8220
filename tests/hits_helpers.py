"""Shared by the hit-query tests (test_hits_host.py, test_gpu_hits.py): the reference's answers, composed on the CPU.

The oracle's known-answer entries (oracle.kat: orc_kat_sphere / orc_kat_triangle / orc_kat_plane) evaluate one
object's trace() for one ray, with and without out-parameters.  ``compose`` forms the (object x ray) table of a scene
description and reads the two answers off it as Scene::trace does: the closest hit is the first minimum of the
distances over the objects in insertion order (Scene.cpp:82-107: strict `<` from FLT_MAX -- np.argmin's rule), the
any-hit the OR of the shadow flags over every object but ``skip`` (Scene.cpp:133-143).
"""
from __future__ import annotations

import numpy as np

import oracle as orc
from rays_helpers import incoherent_rays, scene

FLT_MAX = np.float32(3.4028234663852886e38)
PLANES = ("object", "distance", "point", "normal", "reflected", "colour")
KIND = {"sphere": 0, "triangle": 1, "plane": 2}
_TABLE, _COMPOSED = {}, {}


def table(desc, rays):
    """(hit records (objects, n, 15) float32 in oracle.kat's layout, colours (objects, n, 3)): every object against
    every ray.  The colour is the scene description's, or -- a textured triangle -- the known-answer entry's texel."""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    n, objs = rays.shape[0], desc.objects
    out = np.zeros((len(objs), n, 15), np.float32)
    col = np.zeros((len(objs), n, 3), np.float32)
    tex_of = {oi: (ti, uv) for (oi, ti, uv) in desc.settex}

    def run(kind, idx, params, tex=None, textured=False):
        if not idx:
            return
        p = np.asarray(params, np.float32)
        rec = np.concatenate([np.broadcast_to(rays[None], (len(idx), n, 6)),
                              np.broadcast_to(p[:, None, :], (len(idx), n, p.shape[1]))], axis=2)
        res = orc.kat(kind, rec.reshape(len(idx) * n, -1), tex=tex, textured=textured).reshape(len(idx), n, 15)
        out[idx] = res
        if textured:
            col[idx] = res[:, :, 11:14]

    sph = [j for j, ob in enumerate(objs) if ob[0] == "sphere"]
    run("sphere", sph, [list(objs[j][1]) + [objs[j][2], 0.0] for j in sph])
    pln = [j for j, ob in enumerate(objs) if ob[0] == "plane"]
    run("plane", pln, [list(objs[j][1]) + list(objs[j][2]) for j in pln])
    tri = [j for j, ob in enumerate(objs) if ob[0] == "triangle"]
    plain = [j for j in tri if j not in tex_of]
    run("triangle", plain, [list(objs[j][1]) + list(objs[j][2]) + list(objs[j][3]) + [0.0] * 6 for j in plain])
    for ti in sorted({tex_of[j][0] for j in tri if j in tex_of}):
        idx = [j for j in tri if j in tex_of and tex_of[j][0] == ti]
        run("triangle", idx, [list(objs[j][1]) + list(objs[j][2]) + list(objs[j][3]) + list(tex_of[j][1]) for j in idx],
            tex=desc.textures[ti].argb, textured=True)
    for j, ob in enumerate(objs):
        if j not in tex_of or ob[0] != "triangle":
            col[j] = np.asarray(ob[-1][1], np.float32)
    return out, col


def closest(tab, col):
    """The six planes of rfx_query_hits from a table: dict of arrays, misses as the entry point writes them."""
    out, n = tab, tab.shape[1]
    dist = np.where(out[:, :, 0] > 0, out[:, :, 10], np.float32(np.inf))
    win = np.argmin(dist, axis=0)  # the first minimum: insertion order, strict `<`
    ar = np.arange(n)
    hit = np.isfinite(dist[win, ar])
    rec = out[win, ar]
    z3 = np.zeros((n, 3), np.float32)
    h3 = hit[:, None]
    return {
        "object": np.where(hit, win, -1).astype(np.int32),
        "distance": np.where(hit, rec[:, 10], FLT_MAX).astype(np.float32),
        "point": np.where(h3, rec[:, 1:4], z3),
        "normal": np.where(h3, rec[:, 4:7], z3),
        "reflected": np.where(h3, rec[:, 7:10], z3),
        "colour": np.where(h3, col[win, ar], z3),
    }


def any_hit(tab, skip=None):
    """rfx_query_occluded from a table: uint8 per ray; skip: per-ray object index left out (None, or values outside
    [0, objects): nothing)."""
    flags = tab[:, :, 14] > 0
    if skip is not None:
        skip = np.asarray(skip, np.int64)
        ok = (skip >= 0) & (skip < tab.shape[0])
        flags = flags.copy()
        flags[skip[ok], np.flatnonzero(ok)] = False
    return flags.any(axis=0).astype(np.uint8)


def compose(desc, rays, key=None):
    """(closest-hit planes, table) for a scene description and rays; key: cache the result under it."""
    if key is not None and key in _COMPOSED:
        return _COMPOSED[key]
    tab, col = table(desc, rays)
    res = (closest(tab, col), tab)
    for a in list(res[0].values()) + [tab]:
        a.setflags(write=False)
    if key is not None:
        _COMPOSED[key] = res
    return res


def incoherent(name):
    """compose() on rays_helpers.incoherent_rays(name), computed once per scene."""
    return compose(scene(name), incoherent_rays(name), key=("incoherent", name))


def kinds(desc, objects):
    """[spheres, triangles, planes, misses] among the winners ``objects``."""
    k = np.array([KIND[ob[0]] for ob in desc.objects])
    objects = np.asarray(objects)
    won = k[objects[objects >= 0]]
    return [int((won == 0).sum()), int((won == 1).sum()), int((won == 2).sum()), int((objects < 0).sum())]


def same_bits(got, want):
    """Indices of the rays where two planes differ in any bit."""
    g = np.ascontiguousarray(got).reshape(len(got), -1)
    w = np.ascontiguousarray(want).reshape(len(want), -1)
    assert g.dtype.itemsize == w.dtype.itemsize and g.shape == w.shape, (g.dtype, w.dtype, g.shape, w.shape)
    u = {1: np.uint8, 4: np.uint32}[g.dtype.itemsize]
    return np.flatnonzero((g.view(u) != w.view(u)).any(axis=1))
