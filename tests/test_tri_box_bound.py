"""The BVH box test (rfx_bvh.h ray_inv, bvh_box) keeps the box of every triangle a ray is reported to hit.

The triangle tree (rfx_scene.cpp build_tri_tree) holds the triangles whose basis has cond < 300; a child box is the
AABB of its triangles' vertices, widened like the sphere boxes by kCullRel (|o - centre| + half-diagonal) + 1e-6.
That is sound if a ray the reference's float test (Triangle.cpp:53-108) reports as a hit passes within that margin of
the vertices' box.  This test takes the reference's verdict from the oracle's triangle known-answer entry
(oracle.kat("triangle", ...)) on 2^20 rays aimed within 1e-7 .. 1e-2 (relative to the distance) of the edges and
vertices of triangles with cond spread over [1, 300), from origins 0.05 .. 2000 triangle sizes away, and asserts for
every reported hit that the float32 replay of the kernel's box test (tests/test_bvh_box_bound.py kept: pre-widened
boxes, fused slabs) keeps the triangle's own AABB -- the tightest box any node above it can have.  It also measures how far
outside that AABB a reported hit's crossing point lies, relative to |o - centre| + half-diagonal: the excursion the
margin must cover (bound: 1.25e-3, which kCullRel = 2e-3 covers 1.6 times; observed: DESIGN.md "Triangle BVH").
"""
import numpy as np
import pytest

from test_bvh_box_bound import F, kept

BOUND = 1.25e-3
N = 1 << 20
_CASE = {}


def case():
    """rays, triangles and the reference's verdicts, computed once"""
    if _CASE:
        return _CASE
    import oracle as orc
    rng = np.random.default_rng(20261019)
    n = N
    size = np.exp(rng.uniform(np.log(0.02), np.log(60.0), n))
    ratio = np.exp(rng.uniform(np.log(0.02), 0.0, n))
    ang = rng.uniform(np.radians(3.0), np.radians(177.0), n)
    # an orthonormal frame (e1, e2, e3) per triangle; every 8th triangle axis-aligned (a flat box, like a ground quad)
    q = rng.normal(size=(n, 3, 3))
    e1 = q[:, 0] / np.linalg.norm(q[:, 0], axis=1)[:, None]
    e2 = q[:, 1] - (q[:, 1] * e1).sum(1)[:, None] * e1
    e2 /= np.linalg.norm(e2, axis=1)[:, None]
    flat = np.arange(n) % 8 == 0
    e1[flat] = (1.0, 0.0, 0.0)
    e2[flat] = (0.0, 0.0, 1.0)
    v0 = rng.uniform(-30.0, 30.0, (n, 3))
    ea = e1 * size[:, None]
    eb = (e1 * np.cos(ang)[:, None] + e2 * np.sin(ang)[:, None]) * (size * ratio)[:, None]
    V = np.stack([v0, v0 + ea, v0 + eb], axis=1).astype(F).astype(np.float64)   # the float vertices are the triangle
    a, b = V[:, 2] - V[:, 0], V[:, 1] - V[:, 0]                                   # the reference's basis columns
    nrm = np.cross(b, a)
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    M = np.stack([a, b, -nrm], axis=2)
    cond = np.linalg.norm(M, axis=(1, 2)) * np.linalg.norm(np.linalg.inv(M), axis=(1, 2))
    # a target on an edge (a random point of it) or at a vertex, moved in the plane across the edge by eps * distance
    k = rng.integers(0, 3, n)
    A, B = V[np.arange(n), k], V[np.arange(n), (k + 1) % 3]
    s = np.where(rng.random(n) < 0.3, 0.0, rng.random(n))
    p = A + (B - A) * s[:, None]
    out = np.cross(B - A, nrm)
    out /= np.linalg.norm(out, axis=1)[:, None]
    dist = size * np.exp(rng.uniform(np.log(0.05), np.log(2000.0), n))
    eps = rng.normal(0.0, 1.0, n) * np.exp(rng.uniform(np.log(1e-7), np.log(1e-2), n))
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    o = p + u * dist[:, None]
    ray = (p + out * (eps * dist)[:, None] - o) * np.exp(rng.uniform(np.log(0.1), np.log(10.0), n))[:, None]
    rec = np.zeros((n, 21), F)
    rec[:, 0:3], rec[:, 3:6] = o, ray
    rec[:, 6:15] = V.reshape(n, 9)
    res = orc.kat("triangle", rec)
    hit = (res[:, 0] != 0) | (res[:, 14] != 0)
    _CASE.update(o=rec[:, 0:3].copy(), ray=rec[:, 3:6].copy(), V=V, cond=cond, hit=hit, nrm=nrm)
    return _CASE


def test_cases_cover_the_tree_s_triangles():
    c = case()
    tree = c["cond"] < 300.0
    assert tree.sum() > N // 2 and (c["hit"] & tree).sum() > N // 8
    for lo, hi in ((1.0, 10.0), (10.0, 100.0), (100.0, 300.0)):   # cond spread over [1, 300)
        assert ((c["cond"] >= lo) & (c["cond"] < hi) & c["hit"]).sum() > N // 100, (lo, hi)


@pytest.mark.parametrize("form", ["prewide"])  # (the one form the kernels have; the id and the seed are its own)
def test_box_test_keeps_the_box_of_every_reported_triangle(form):
    c = case()
    sel = c["hit"] & (c["cond"] < 300.0)
    V, o, d = c["V"][sel], c["o"][sel], c["ray"][sel]
    n = len(V)
    rng = np.random.default_rng(5 + 2)
    lo, hi = V.min(1), V.max(1)                                  # exact in float: the vertices are floats
    centre, half_diag = 0.5 * (lo + hi), 0.5 * np.linalg.norm(hi - lo, axis=1)
    ref = centre + rng.uniform(-15.0, 15.0, (n, 3))              # the trees' margin reference point
    mt = np.nextafter(((np.linalg.norm(ref - centre, axis=1) + half_diag) * 1.0001).astype(F), F(np.inf))
    k = kept(lo.astype(F), hi.astype(F), o, d, ref.astype(F), mt, rng)
    assert k.all(), int((~k).sum())


def test_reported_hits_stay_inside_the_margin_of_the_vertex_box():
    c = case()
    sel = c["hit"] & (c["cond"] < 300.0)
    V, nrm = c["V"][sel], c["nrm"][sel]
    o, d = c["o"][sel].astype(np.float64), c["ray"][sel].astype(np.float64)
    t = ((V[:, 0] - o) * nrm).sum(1) / (d * nrm).sum(1)          # the exact crossing of the triangle's plane
    P = o + d * t[:, None]
    lo, hi = V.min(1), V.max(1)
    outside = np.linalg.norm(np.maximum(np.maximum(lo - P, P - hi), 0.0), axis=1)
    scale = np.linalg.norm(o - 0.5 * (lo + hi), axis=1) + 0.5 * np.linalg.norm(hi - lo, axis=1)
    worst = float((outside / scale).max())
    print(f"worst excursion of a reported hit outside its vertex box: {worst:.3e} of |o - centre| + half-diagonal "
          f"({int(sel.sum())} reported hits; bound {BOUND:.2e}, kCullRel 2e-3)")
    assert worst < BOUND
