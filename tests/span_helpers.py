"""Shared by the span-query tests (test_span_host.py, test_gpu_span.py): the reference's answers on a per-ray
interval, composed on the CPU from hits_helpers.table().

A candidate of ray i is an object whose out-parameter trace() returns true (table column 0), at the float distance it
reports (column 10).  It is eligible iff dist <= hi[i] and (dist, object) > (lo[i], after[i]) lexicographically --
plain float32 comparisons (rfx.h "Ray intervals").  closest_span is hits_helpers.closest on the eligible candidates,
any_hit_span the OR of the eligible candidates but ``skip``, layers the candidates in ascending (dist, index).
"""
from __future__ import annotations

import numpy as np

from hits_helpers import FLT_MAX, compose
from rays_helpers import NRAYS, scene, scene_box

INT32_MAX = np.int32(2 ** 31 - 1)
_RAYS = {}


def pierce_rays(name, n=NRAYS):
    """n rays from outside the scene's box through a point of one of its objects: several hits per ray."""
    if ("pierce", name) in _RAYS:
        return _RAYS[("pierce", name)]
    desc = scene(name)
    g = np.random.default_rng(20261021)
    lo, hi = scene_box(desc)
    c, diag = (lo + hi) / 2, np.linalg.norm(hi - lo)
    objs = [ob for ob in desc.objects if ob[0] != "plane"]
    u = g.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    u[:, 1] = np.abs(u[:, 1]) + 0.05
    o = c + 0.75 * diag * u
    t = np.empty((n, 3))
    for i in range(n):
        ob = objs[int(g.integers(len(objs)))]
        if ob[0] == "sphere":
            v = g.normal(size=3)
            t[i] = np.array(ob[1]) + 0.5 * ob[2] * v / np.linalg.norm(v)
        else:
            w = g.dirichlet(np.ones(3))
            t[i] = w[0] * np.array(ob[1]) + w[1] * np.array(ob[2]) + w[2] * np.array(ob[3])
    d = t - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d *= 10.0 ** g.uniform(-2.0, 2.0, (n, 1))
    rays = np.concatenate([o, d], axis=1).astype(np.float32)
    rays.setflags(write=False)
    _RAYS[("pierce", name)] = rays
    return rays


def far(rays, back):
    """The same lines from ``back`` units behind, unit directions: the distances crowd into tri_takes' 2^-20 band."""
    r = rays.astype(np.float64)
    u = r[:, 3:6] / np.linalg.norm(r[:, 3:6], axis=1, keepdims=True)
    r[:, 0:3] -= back * u
    r[:, 3:6] = u
    return r.astype(np.float32)


def pierce(name):
    """(closest-hit planes, table, colours) on pierce_rays(name), computed once per scene."""
    return composed(name, "pierce")


def composed(name, kind, desc=None, rays=None):
    """(planes, table, colours) of a named ray set of a scene, computed once: kind "pierce", "far" (far(pierce, 1e6)),
    "incoherent", or any other name with ``rays`` given."""
    from hits_helpers import table
    from rays_helpers import incoherent_rays
    key = ("span", kind, name)
    if key not in _RAYS:
        if rays is None:
            rays = {"pierce": lambda: pierce_rays(name), "far": lambda: far(pierce_rays(name), 1e6),
                    "incoherent": lambda: incoherent_rays(name)}[kind]()
        d = desc if desc is not None else scene(name)
        planes, tab = compose(d, rays, key=key)
        # hits_helpers.table's colour table (compose does not keep it): the description's colour, or -- a textured
        # triangle -- the table's own texel columns
        col = np.zeros(tab.shape[:2] + (3,), np.float32)
        tex_of = {oi for (oi, ti, uv) in d.settex}
        for j, ob in enumerate(d.objects):
            col[j] = tab[j, :, 11:14] if (j in tex_of and ob[0] == "triangle") else np.asarray(ob[-1][1], np.float32)
        col.setflags(write=False)
        _RAYS[key] = (planes, tab, col)
    return _RAYS[key]


def _dist(tab):
    """(objects, n) float32 distances, +inf where the object is no candidate."""
    return np.where(tab[:, :, 0] > 0, tab[:, :, 10], np.float32(np.inf)).astype(np.float32)


def eligible(tab, lo=None, after=None, hi=None):
    """(objects, n) bool: the candidates inside each ray's interval.  Scalars hold for every ray."""
    dist = _dist(tab)
    m, n = dist.shape
    ok = np.isfinite(dist)
    j = np.arange(m, dtype=np.int64)[:, None]
    with np.errstate(invalid="ignore"):
        if hi is not None:
            ok &= dist <= np.broadcast_to(np.asarray(hi, np.float32), (n,))[None, :]
        if lo is not None:
            lo = np.broadcast_to(np.asarray(lo, np.float32), (n,))[None, :]
            af = np.broadcast_to(np.asarray(-1 if after is None else after, np.int64), (n,))[None, :]
            ok &= (dist > lo) | ((dist == lo) & (j > af))
    return ok


def _planes(tab, col, win, hit):
    n = tab.shape[1]
    ar = np.arange(n)
    rec = tab[win, ar]
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


def closest_span(tab, col, lo=None, after=None, hi=None):
    """The six planes of rfx_query_hits_span: the first minimum of the distance over the eligible candidates."""
    d = np.where(eligible(tab, lo, after, hi), _dist(tab), np.float32(np.inf))
    win = np.argmin(d, axis=0)
    return _planes(tab, col, win, np.isfinite(d[win, np.arange(tab.shape[1])]))


def any_hit_span(tab, skip=None, lo=None, hi=None):
    """rfx_query_occluded_span: uint8 per ray, 1 iff an eligible candidate other than skip[i] exists."""
    ok = eligible(tab, lo, None, hi)
    if skip is not None:
        skip = np.broadcast_to(np.asarray(skip, np.int64), (tab.shape[1],))
        valid = (skip >= 0) & (skip < tab.shape[0])
        ok[skip[valid], np.flatnonzero(valid)] = False
    return ok.any(axis=0).astype(np.uint8)


def layers(tab, col, k):
    """k dicts of planes: layer l is each ray's l-th candidate in ascending (dist, index) (np.lexsort: the last key
    is the primary one), a miss where the ray has fewer."""
    d = _dist(tab)
    m, n = d.shape
    idx = np.broadcast_to(np.arange(m)[:, None], (m, n))
    out = []
    order = np.lexsort((idx, d), axis=0)  # per ray (column): rows sorted by d, then by index
    for l in range(k):
        if l < m:
            win = order[l]
            hit = np.isfinite(d[win, np.arange(n)])
        else:
            win, hit = np.zeros(n, np.int64), np.zeros(n, bool)
        out.append(_planes(tab, col, win, hit))
    return out


def counts(tab):
    """Candidates per ray."""
    return (tab[:, :, 0] > 0).sum(axis=0)


def band_pairs(tab):
    """(rays whose two nearest distances lie within 2^-20 relative, rays where they are the same float)."""
    d = np.sort(_dist(tab), axis=0)
    if d.shape[0] < 2:
        return 0, 0
    two = np.isfinite(d[1])
    a, b = d[0][two].astype(np.float64), d[1][two].astype(np.float64)
    return int(((b - a) <= b * 2.0 ** -20).sum()), int((a == b).sum())
