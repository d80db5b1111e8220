"""Shared by the bundle-cull tests (test_bundle_cull_bound.py, test_gpu_bundle_cull.py).

A float32 numpy restatement of rfx_bundle.h in the default build's form (RFX_CULL_FMA 1): make_bundle, make_bundle_ball,
make_bundle_quad, the cone term of cull_chunk / cull_small, cull_small's plane rule (`away`) and tri_footprint_misses,
operation for operation: fused sums through float64 (test_bvh_box_bound.fmaf), v_rsq_f32 / v_sqrt_f32 / v_rcp_f32
within 1 ulp of the rounded value (test_bvh_box_bound.approx).  The host records come from the library itself
(rfx_scene_cull_dump), never from a restatement.  And the generators of the wave bundles the tests use: 64 coherent
rays next to the silhouette of a triangle or sphere (aimed), leaving a triangle's plane while heading over it
(departing), with scattered origins (spread), a light's shadow ball and a pixel's sample quadrilateral.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from test_bvh_box_bound import F, approx, fmaf

K_CULL_REL = F(2e-3)      # rfx_bundle.h kCullRel
AWAY_REL = F(1e-3)        # cull_small: the 1e-3 of ms and ma
FOOT_REL = F(1e-2)        # tri_footprint_misses: the 1e-2 of m
CLASSES = ((3.0, 100.0), (100.0, 300.0), (300.0, np.inf))  # cond classes: footprint + plane, plane only, never culled


# ------------------------------------------------------------------------------------------ float32 building blocks
def cdot(a, b):
    """rfx_bundle.h cdot: fma(az, bz, fma(ay, by, ax bx))"""
    a, b = np.broadcast_arrays(a, b)
    return fmaf(a[..., 2], b[..., 2], fmaf(a[..., 1], b[..., 1], a[..., 0] * b[..., 0]))


def pdot(a, b):
    """the unfused sum ax bx + ay by + az bz"""
    a, b = np.broadcast_arrays(a, b)
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def rsq(x, rng):
    with np.errstate(divide="ignore", invalid="ignore"):
        return approx(1.0 / np.sqrt(x.astype(np.float64)), rng)


def sqrt(x, rng):
    with np.errstate(invalid="ignore"):
        return approx(np.sqrt(x.astype(np.float64)), rng)


def rcp(x, rng):
    with np.errstate(divide="ignore"):
        return approx(1.0 / x.astype(np.float64), rng)


def _first_live(live):
    return np.argmax(live, axis=1)


def _finish(B, e2, dev, bad, live, rng):
    """the shared tail of the three make_bundle forms: wave maxima, widening, B.ok"""
    e2m = np.where(live, e2, F(0)).max(1)
    devm = np.where(live, np.fmax(dev, F(0)), F(0)).max(1)
    nan = (live & (np.isnan(e2) | np.isnan(dev))).any(1)   # wave_max_nonneg: a NaN pattern wins
    B.rw = sqrt(e2m, rng) * F(1.0001)
    B.cosa = F(1) - devm - F(4e-6)
    B.sina = sqrt(np.fmax(F(1) - B.cosa * B.cosa, F(0)) + F(1e-7), rng) * F(1.001)
    with np.errstate(invalid="ignore"):
        B.ok = ~bad.any(1) & ~nan & (B.cosa > F(0.1)) & (B.rw <= F(1e15))
    return B


def make_bundle(o, d, live, rng):
    """rfx_bundle.h make_bundle.  o, d: (n, 64, 3) float32; live: (n, 64) bool, at least one per row."""
    n = len(o)
    ref = _first_live(live)
    B = SimpleNamespace(c=o[np.arange(n), ref])
    d0 = d[np.arange(n), ref]
    B.a = d0 * rsq(cdot(d0, d0), rng)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        e = o - B.c[:, None, :]
        e2 = cdot(e, e)
        cosl = cdot(d, B.a[:, None, :]) * rsq(cdot(d, d), rng)
        dev = F(1) - cosl
        bad = live & ~((e2 <= F(1e30)) & (dev >= F(-0.5)) & (dev <= F(2.5)))
    return _finish(B, e2, dev, bad, live, rng)


def make_bundle_ball(o, d, R, live, rng):
    """rfx_bundle.h make_bundle_ball: every ray (o, d + rd R), |rd| <= 1.  R: (n,) float32."""
    n = len(o)
    ref = _first_live(live)
    B = SimpleNamespace(c=o[np.arange(n), ref])
    d0 = d[np.arange(n), ref]
    B.a = d0 * rsq(pdot(d0, d0), rng)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        e = o - B.c[:, None, :]
        e2 = pdot(e, e)
        idl = rsq(pdot(d, d), rng)
        ca = np.fmin(pdot(d, B.a[:, None, :]) * idl, F(1))
        sa = sqrt(np.fmax(F(1) - ca * ca, F(0)), rng)
        sb = np.fmin(R[:, None] * idl * F(1.001), F(1))
        cb = sqrt(np.fmax(F(1) - sb * sb, F(0)), rng)
        dev = F(1) - (ca * cb - sa * sb)
        bad = live & ~((e2 <= F(1e30)) & (dev >= F(-0.5)) & (dev <= F(2.5)) & (sb < F(0.5)))
    B = _finish(B, e2, dev, bad, live, rng)
    B.sb = sb
    return B


def make_bundle_quad(o, dq, live, rng):
    """rfx_bundle.h make_bundle_quad: every ray from o inside the quadrilateral dq[:, :, 0..3].  dq: (n, 64, 4, 3)."""
    n = len(o)
    ref = _first_live(live)
    B = SimpleNamespace(c=o[np.arange(n), ref])
    d0 = dq[np.arange(n), ref, 0]
    B.a = d0 * rsq(pdot(d0, d0), rng)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        e = o - B.c[:, None, :]
        e2 = pdot(e, e)
        dev = np.zeros(o.shape[:2], F)
        bad = np.zeros(o.shape[:2], bool)
        for k in range(4):
            v = dq[:, :, k]
            dk = F(1) - pdot(v, B.a[:, None, :]) * rsq(pdot(v, v), rng)
            bad |= ~((dk >= F(-0.5)) & (dk <= F(2.5)))
            dev = np.fmax(dev, dk)
        bad = live & (bad | ~(e2 <= F(1e30)))
    return _finish(B, e2, dev, bad, live, rng)


def cull_terms(rec, B, rng, k_rel=K_CULL_REL, away_rel=AWAY_REL):
    """The cone term (cull_chunk and cull_small share it) and cull_small's plane rule for records rec (n, m, 8) -- or
    (n, m, 4) bounds: the cone alone -- against bundles B (n).  Returns the intermediates by name; `cone` and `away`
    are the two drop decisions (B.ok is the caller's)."""
    c, a = B.c[:, None, :], B.a[:, None, :]
    rw, cosa, sina = B.rw[:, None], B.cosa[:, None], B.sina[:, None]
    T = SimpleNamespace()
    with np.errstate(invalid="ignore", over="ignore"):
        v = rec[..., 0:3] - c
        L2 = cdot(v, v)
        T.L = sqrt(L2, rng)
        r = rec[..., 3]
        T.rp = fmaf(np.broadcast_to(F(k_rel), T.L.shape), T.L + rw, r + rw)
        T.va = cdot(v, a)
        T.lim = fmaf(np.broadcast_to(cosa, T.L.shape), sqrt(np.fmax(fmaf(-T.rp, T.rp, L2), F(0)), rng), -(sina * T.rp))
        T.cone = (T.L > T.rp) & (T.va < T.lim)
        if rec.shape[-1] >= 8:
            nrm = rec[..., 4:7]
            T.side = cdot(nrm, c) - rec[..., 7]
            T.an = cdot(nrm, a)
            T.ms = rw + F(away_rel) * (T.L + r + rw) + F(1e-6)
            T.ma = np.broadcast_to(sina + F(away_rel), T.L.shape)
            T.away = ((T.side > T.ms) & (T.an > T.ma)) | ((T.side < -T.ms) & (T.an < -T.ma))
    return T


def cull_chunk(bound, B, rng):
    """rfx_bundle.h cull_chunk: keep bits (n, m) of bounds (n, m, 4)"""
    return ~cull_terms(bound, B, rng).cone


def tri_footprint_misses(q, side, an, B, rng, foot_rel=FOOT_REL):
    """rfx_bundle.h tri_footprint_misses for footprint records q (n, m, 12); side, an (n, m) from cull_terms.
    Returns (misses, used): used = the largest of the three conditions' value / margin ratios (> 1: it misses)."""
    c, a = B.c[:, None, :], B.a[:, None, :]
    rw, cosa, sina = B.rw[:, None], B.cosa[:, None], B.sina[:, None]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        h = np.abs(side)
        anp = np.where(side > 0, -an, an)
        snp = sqrt(np.fmax(F(1) - anp * anp, F(0)), rng)
        ndmin = anp * cosa - snp * sina
        gate = (h > rw * F(1.01) + F(1e-4)) & (ndmin > F(0.1))
        ind, ian = rcp(ndmin, rng) * F(1.001), rcp(anp, rng) * F(1.001)
        tp = h * ian * (F(1) / F(1.001))
        p = (c + tp[..., None] * a) - q[..., 0:3]
        chord = sqrt(np.fmax(F(2) - F(2) * cosa, F(0)), rng) * F(1.001)
        R = (h * chord * (F(1) + ian) * ind + rw * (F(1) + ind) + F(1e-4) * tp) * F(1.001) + F(1e-6)
        cv = c - q[..., 0:3]
        mag = sqrt(pdot(cv, cv), rng) * F(1.001) + rw + (h + rw) * ind
        m = F(foot_rel) * mag + F(1e-6)
        nu, nv, nuv = q[..., 3], q[..., 7], q[..., 11]
        u0, v0 = pdot(q[..., 4:7], p), pdot(q[..., 8:11], p)
        mu, mv, muv = (R + m) * nu, (R + m) * nv, R * nuv + m * (nu + nv)
        miss = (u0 + mu < F(0)) | (v0 + mv < F(0)) | (u0 + v0 - R * nuv - m * (nu + nv) > F(1))
        used = np.fmax(np.fmax(-u0 / mu, -v0 / mv), (u0 + v0 - F(1)) / muv)
        used = np.where(gate & np.isfinite(used), used, F(0))
    return gate & miss, used


def cull_small(recs, tris, valid, B, rng, foot=False, **kw):
    """rfx_bundle.h cull_small<FOOT>: keep bits (n, 64) bool for the lane records recs (64, 8) or (n, 64, 8), the
    footprint records tris (32, 12) or (n, 32, 12) and the valid lanes (an int or (n,) of them).  Without B.ok the
    callers take `valid` (every kernel: `B.ok ? cull_small(...) : S.cull_valid`), and so does this."""
    n = len(B.rw)
    recs = np.broadcast_to(recs, (n, 64, 8))
    T = cull_terms(recs, B, rng, **kw)
    keep = ~T.cone & ~T.away
    if foot:
        miss, _ = tri_footprint_misses(np.broadcast_to(tris, (n, 32, 12)), T.side[:, 32:], T.an[:, 32:], B, rng)
        keep[:, 32:] &= ~miss
    v = np.asarray(valid, np.uint64).reshape(-1, 1)
    vb = ((v >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    return np.where(B.ok[:, None], keep, True) & vb


# ------------------------------------------------------------------------------------------ triangles and records
def triangles(n, seed):
    """test_tri_box_bound.case()'s recipe: size 0.02 .. 60, aspect 0.02 .. 1, angle 3 .. 177 degrees, random frames,
    every 8th axis-aligned.  Returns V (n, 3, 3) float64 holding float32 values, the unit normal, cond, the bounding
    radius about the centroid."""
    rng = np.random.default_rng(seed)
    size = np.exp(rng.uniform(np.log(0.02), np.log(60.0), n))
    ratio = np.exp(rng.uniform(np.log(0.02), 0.0, n))
    ang = rng.uniform(np.radians(3.0), np.radians(177.0), n)
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
    V = np.stack([v0, v0 + ea, v0 + eb], axis=1).astype(F).astype(np.float64)
    return geometry(V)


def geometry(V):
    a, b = V[:, 2] - V[:, 0], V[:, 1] - V[:, 0]                                   # the reference's basis columns
    nrm = np.cross(b, a)
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    M = np.stack([a, b, -nrm], axis=2)
    cond = np.linalg.norm(M, axis=(1, 2)) * np.linalg.norm(np.linalg.inv(M), axis=(1, 2))
    cen = V.mean(1)
    rad = np.linalg.norm(V - cen[:, None], axis=2).max(1)
    return SimpleNamespace(V=V, nrm=nrm, cond=cond, cen=cen, rad=rad, size=np.linalg.norm(b, axis=1))


def cond_class(cond):
    """index into CLASSES (cond below 3 counts with the first)"""
    return (cond >= 100.0).astype(int) + (cond >= 300.0).astype(int)


def library_records(V=None, spheres=None):
    """The library's own cull records, in scenes of 32 triangles V (n, 3, 3) and / or 32 spheres (n, 4) through
    rfx_scene_add_triangle / rfx_scene_add_sphere and rfx_scene_cull_dump: (triangle lane records (n, 8), footprint
    records (n, 12), sphere lane records (n, 8)), None where none were given."""
    from reflaxman_amd.render import Color, Material, Scene, Vector3
    mat = Material()
    n = len(V) if V is not None else len(spheres)
    recs, tris, srec = np.zeros((n, 8), F), np.zeros((n, 12), F), np.zeros((n, 8), F)
    for first in range(0, n, 32):
        s = Scene(Color(1, 1, 1), 0.1)
        m = min(32, n - first)
        want = 0
        if spheres is not None:
            for c in spheres[first:first + m]:
                s.addSphere(Vector3(*[float(x) for x in c[:3]]), float(c[3]), mat)
            lanes = [(i & 1) * 16 + (i >> 1) for i in range(m)]
            want |= sum(1 << l for l in lanes)
        if V is not None:
            for t in V[first:first + m]:
                s.addTriangle(*[Vector3(*[float(x) for x in v]) for v in t], mat)
            want |= ((1 << m) - 1) << 32
        r, q, valid = s.cull_dump()
        assert valid == want, (hex(valid), hex(want))
        if spheres is not None:
            srec[first:first + m] = r[lanes]
        if V is not None:
            recs[first:first + m], tris[first:first + m] = r[32:32 + m], q[:m]
    return (recs if V is not None else None, tris if V is not None else None, srec if spheres is not None else None)


# ------------------------------------------------------------------------------------------ bundles
_II, _JJ = (g.reshape(-1) for g in np.meshgrid(np.arange(8) - 3.5, np.arange(8) - 3.5))


def _grid(c, w1, w2, step):
    """64 directions: c plus an 8 x 8 grid of steps along w1, w2 (float64, (n, 64, 3))"""
    return c[:, None, :] + (w1[:, None, :] * _II[None, :, None] + w2[:, None, :] * _JJ[None, :, None]) * step[:, None, None]


def _unit(v):
    return v / np.linalg.norm(v, axis=-1)[..., None]


def _scatter(rng, o, d, dist, converge):
    """spread origins: the 64 origins scattered over a patch of 1e-4 .. 1e-1 of the distance (rw > 0, as for secondary
    and shadow bundles); converge: the rays keep their targets (shadow-like), else their directions (mirror-like)"""
    n = len(o)
    patch = np.exp(rng.uniform(np.log(1e-4), np.log(1e-1), n)) * dist
    off = rng.normal(size=(n, 64, 3))
    off *= (rng.random((n, 64)) ** (1 / 3) / np.linalg.norm(off, axis=2))[..., None] * patch[:, None, None]
    off[:, 0] = 0.0
    o = o[:, None, :] + off
    return o, np.where(converge[:, None, None], d - off, d)


def aimed(p, out, nrm, size, seed, spread=False):
    """Bundles whose axis points at a spot within +-4 pixels of the silhouette point p (n, 3) of the target (out: the
    outward direction in the silhouette's plane, nrm: the plane's normal, size: the target's).  The eye is 0.05 ..
    2000 sizes away; half of the eyes graze the plane at a height of 1e-4 .. 1e-1 of the distance, on either side;
    pixel angle 1e-5 .. 3e-2 rad, lanes on an 8 x 8 grid.  Returns (o, d) float32 (n, 64, 3)."""
    rng = np.random.default_rng(seed)
    n = len(p)
    dist = size * np.exp(rng.uniform(np.log(0.05), np.log(2000.0), n))
    u = _unit(rng.normal(size=(n, 3)))
    tang = _unit(u - (u * nrm).sum(1)[:, None] * nrm)
    hrel = np.exp(rng.uniform(np.log(1e-4), np.log(1e-1), n)) * rng.choice([-1.0, 1.0], n)
    u = np.where((rng.random(n) < 0.5)[:, None], _unit(tang + nrm * hrel[:, None]), u)
    o = p + u * dist[:, None]
    pix = np.exp(rng.uniform(np.log(1e-5), np.log(3e-2), n))
    eps = np.clip(rng.normal(0.0, 1.5, n), -4.0, 4.0) * pix
    return _lanes(rng, o, p + out * (eps * dist)[:, None] - o, pix, dist, spread)


def _lanes(rng, o, c, pix, dist, spread):
    """the 64 rays of each bundle: axis c from eye o, lanes on an 8 x 8 grid of pixel angle pix"""
    n = len(o)
    cl = np.linalg.norm(c, axis=1)
    w1 = _unit(np.cross(c, rng.normal(size=(n, 3))))
    w2 = _unit(np.cross(c, w1))
    d = _grid(c, w1, w2, pix * cl)
    o = np.broadcast_to(o[:, None, :], d.shape)
    if spread:
        o, d = _scatter(rng, o[:, 0], d, dist, rng.random(n) < 0.5)
    return o.astype(F), d.astype(F)


def aimed_sphere(c, r, seed, spread=False):
    """aimed() for spheres: the eye 0.05 .. 2000 radii off the surface, the axis within +-4 pixels of the tangent cone"""
    rng = np.random.default_rng(seed)
    n = len(c)
    dist = r * np.exp(rng.uniform(np.log(0.05), np.log(2000.0), n))
    u = _unit(rng.normal(size=(n, 3)))
    w = rng.normal(size=(n, 3))
    w = _unit(w - (w * u).sum(1)[:, None] * u)
    L = r + dist
    o = c + u * L[:, None]
    pix = np.exp(rng.uniform(np.log(1e-5), np.log(3e-2), n))
    th = np.arcsin(r / L) + np.clip(rng.normal(0.0, 1.5, n), -4.0, 4.0) * pix
    return _lanes(rng, o, (-u * np.cos(th)[:, None] + w * np.sin(th)[:, None]) * L[:, None], pix, dist, spread)


def tri_silhouette(G, seed):
    """a point on an edge (a random point of it) or at a vertex of each triangle, and the outward in-plane direction"""
    rng = np.random.default_rng(seed)
    n = len(G.V)
    k = rng.integers(0, 3, n)
    A, B = G.V[np.arange(n), k], G.V[np.arange(n), (k + 1) % 3]
    s = np.where(rng.random(n) < 0.3, 0.0, rng.random(n))
    out = _unit(np.cross(B - A, G.nrm))
    inside = ((G.cen - A) * out).sum(1) > 0      # orient `out` away from the centroid
    return A + (B - A) * s[:, None], np.where(inside[:, None], -out, out)


def departing(G, seed, spread=False):
    """Bundles that leave a triangle's plane while heading back over the triangle: the eye at height +-(1e-5 .. 1e-1)
    dist over the plane, dist = 0.05 .. 200 bounding radii along the plane from a point inside the triangle; the axis
    leaves the plane by 1e-5 .. 1e-1; pixel angle 1e-6 .. 1e-2."""
    rng = np.random.default_rng(seed)
    n = len(G.V)
    w = rng.dirichlet([1.0, 1.0, 1.0], n)
    p = (G.V * w[:, :, None]).sum(1)
    u = rng.normal(size=(n, 3))
    tang = _unit(u - (u * G.nrm).sum(1)[:, None] * G.nrm)
    dist = G.rad * np.exp(rng.uniform(np.log(0.05), np.log(200.0), n))
    sgn = rng.choice([-1.0, 1.0], n)
    hrel = np.exp(rng.uniform(np.log(1e-5), np.log(1e-1), n))
    anr = np.exp(rng.uniform(np.log(1e-5), np.log(1e-1), n))
    o = p + tang * dist[:, None] + G.nrm * (sgn * hrel * dist)[:, None]
    c = -tang + G.nrm * (sgn * anr)[:, None]
    pix = np.exp(rng.uniform(np.log(1e-6), np.log(1e-2), n))
    w1 = _unit(np.cross(c, G.nrm))
    w2 = _unit(np.cross(c, w1))
    d = _grid(c, w1, w2, pix) * dist[:, None, None]
    o = np.broadcast_to(o[:, None, :], d.shape)
    if spread:
        o, d = _scatter(rng, o[:, 0], d, dist, rng.random(n) < 0.5)
    return o.astype(F), d.astype(F)


def surface(G, seed):
    """Bundles that start on a triangle's own surface, as a bounce or a shadow ray does: the eye at a point inside the
    triangle, off its plane by +-(1e-8 .. 1e-5) in absolute terms (the rounding of a float hit point at these
    coordinates), the axis 1e-3 .. 1.5 rad off the plane on either side, rays 0.01 .. 1000 bounding radii long, pixel
    angle 1e-6 .. 1e-2.  The record's float side has the sign of its rounding here, and the reference reports
    crossings at any t above 1e-19."""
    rng = np.random.default_rng(seed)
    n = len(G.V)
    w = rng.dirichlet([1.0, 1.0, 1.0], n)
    p = (G.V * w[:, :, None]).sum(1)
    h = np.exp(rng.uniform(np.log(1e-8), np.log(1e-5), n)) * rng.choice([-1.0, 1.0], n)
    o = p + G.nrm * h[:, None]
    u = rng.normal(size=(n, 3))
    tang = _unit(u - (u * G.nrm).sum(1)[:, None] * G.nrm)
    phi = np.exp(rng.uniform(np.log(1e-3), np.log(1.5), n)) * rng.choice([-1.0, 1.0], n)
    c = tang * np.cos(phi)[:, None] + G.nrm * np.sin(phi)[:, None]
    dist = G.rad * np.exp(rng.uniform(np.log(1e-2), np.log(1e3), n))
    pix = np.exp(rng.uniform(np.log(1e-6), np.log(1e-2), n))
    return _lanes(rng, o, c * dist[:, None], pix, dist, False)


def ball_samples(seed=7):
    """16 rd in the unit ball: its centre, its six axis extremes, nine random points (float32)"""
    rng = np.random.default_rng(seed)
    r = _unit(rng.normal(size=(9, 3))) * rng.random((9, 1)) ** (1 / 3) * 0.999
    ax = np.concatenate([np.eye(3), -np.eye(3)])
    return np.concatenate([np.zeros((1, 3)), ax, r]).astype(F)


def shadow_rays(o, d, R, rd):
    """Scene.cpp:128-129 in float32: dropToLight + randDir * lightRadius for each rd: (n, 64, len(rd), 3)"""
    return d[:, :, None, :] + rd[None, None, :, :] * np.asarray(R, F).reshape(-1, 1, 1, 1)


def quad_corners(d, w1, w2):
    """a lane's quadrilateral: its direction moved half a step each way along the grid's two step vectors (float32)"""
    s = np.array([(-0.5, -0.5), (0.5, -0.5), (0.5, 0.5), (-0.5, 0.5)])
    return (d.astype(np.float64)[:, :, None, :] + s[None, None, :, 0, None] * w1[:, None, None, :] +
            s[None, None, :, 1, None] * w2[:, None, None, :]).astype(F)


def quad_rays(dq, seed=11):
    """16 rays bilinearly inside each lane's quadrilateral, the four corners among them: (n, 64, 16, 3) float32"""
    rng = np.random.default_rng(seed)
    st = np.concatenate([[(0, 0), (1, 0), (1, 1), (0, 1)], rng.random((12, 2))])
    s, t = st[:, 0][None, None, :, None], st[:, 1][None, None, :, None]
    q = dq.astype(np.float64)
    lo = q[:, :, None, 0] * (1 - s) + q[:, :, None, 1] * s
    hi = q[:, :, None, 3] * (1 - s) + q[:, :, None, 2] * s
    return (lo * (1 - t) + hi * t).astype(F)


# ------------------------------------------------------------------------------------------ the reference's verdicts
def reported_tri(o, d, V):
    """The reference's float verdict (oracle.kat("triangle")) for rays o, d (n, k, 3) on triangle V (n, 3, 3) each:
    (n, k) bool, a ray reported if its hit flag or its any-hit flag is set."""
    import oracle as orc
    n, k = o.shape[:2]
    rec = np.zeros((n, k, 21), F)
    rec[:, :, 0:3], rec[:, :, 3:6] = o, d
    rec[:, :, 6:15] = V.reshape(n, 1, 9)
    res = orc.kat("triangle", rec.reshape(-1, 21)).reshape(n, k, 15)
    return (res[:, :, 0] != 0) | (res[:, :, 14] != 0)


def reported_sph(o, d, c, r):
    import oracle as orc
    n, k = o.shape[:2]
    rec = np.zeros((n, k, 11), F)
    rec[:, :, 0:3], rec[:, :, 3:6] = o, d
    rec[:, :, 6:9], rec[:, :, 9] = c[:, None, :], r[:, None]
    res = orc.kat("sphere", rec.reshape(-1, 11)).reshape(n, k, 15)
    return (res[:, :, 0] != 0) | (res[:, :, 14] != 0)
