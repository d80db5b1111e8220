"""The closest-hit walkers' distance prune (rfx_bvh.h closest_spheres_bvh, closest_tris_bvh) keeps every child box that
holds a hit no farther than the best one so far -- for rays of any length the reference reports hits at.

A walker skips a child whose widened box the ray enters at parameter t0 when the entry distance t0 |ray| exceeds the
best distance so far: in squares, (t0 |ray|)^2 > h.sq * 1.001.  Written as t0 * t0 * a with a = |ray|^2 the product
leaves float32 at both ends of the lengths a caller may pass (rfx.h: "its direction is used as given"; the reference
reports triangle and plane hits from |ray| ~ 1.1e-19 to ~ 1e19 x distance):

  * |ray| = 1e-18, a box 24 away: t0 = 2.4e19 and t0 * t0 = +inf (the real product is 576);
  * |ray| >= 1.3e19: a = 0.5 * (2 a) = +inf, and t0 * t0 * a = +inf for every t0 > 0;
  * |ray| = 1e19, a box 1e-3 away: t0 * t0 = 1e-44 is a subnormal of 3 significant bits.

In each case the old expression pruned boxes holding the closest hit as soon as h.sq was finite, and the walk returned
the first triangle it met (`prune_before` below restates it; the last test shows it firing).  The kernels now form the
entry distance itself, d0 = t0 * |ray| with |ray| = sqrt(a) for 2^-100 <= a <= 2^100 and 0 (never prune) outside, and
compare d0 * d0: d0 is a scene distance, whose square is a normal float32 wherever h.sq is.

This file restates ray_inv, bvh_box and the prune in float32, as tests/test_bvh_box_bound.py does for the box test,
and checks (1) the `layers` rays of tests/edge_rays.py at every length against the boxes of the triangles the reference
reports as hit, and (2) 2^16 random boxes and rays with |ray| log-uniform over [2^-63, 1e20].
"""
import numpy as np
import pytest

import edge_rays as E

F = np.float32
K_CULL_REL = F(2e-3)  # rfx_bundle.h kCullRel
VERY_SMALL = 2.0 ** -63


def approx(x, rng, ulps=1.0):
    """A hardware approximation (v_rcp_f32 / v_sqrt_f32) within `ulps` ulp of the rounded value."""
    x = x.astype(F)
    return (x.astype(np.float64) * (1.0 + rng.uniform(-ulps, ulps, x.shape) * 2.0 ** -23)).astype(F)


def fmaf(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def slab(lo, hi, o, d, ref, mt, rng):
    """rfx_bvh.h ray_inv + bvh_box for one child in float32: (kept, the entry parameter t0)."""
    e = o - ref
    dm = K_CULL_REL * (approx(np.sqrt((e * e).sum(1, dtype=F)), rng) * F(1.0001)) + F(1e-6)
    with np.errstate(all="ignore"):
        inv = np.clip(approx(F(1) / d, rng), F(-1e30), F(1e30))
        # rfx_scene.cpp: the box grown by kCullRel mt (x (1 + 1e-6)) and rounded outward
        w = 2e-3 * mt.astype(np.float64) * (1.0 + 1e-6)
        lo = np.nextafter((lo.astype(np.float64) - w[:, None]).astype(F), F(-np.inf))
        hi = np.nextafter((hi.astype(np.float64) + w[:, None]).astype(F), F(np.inf))
        a = fmaf(lo, inv, -((o + dm[:, None]) * inv))
        b = fmaf(hi, inv, -((o - dm[:, None]) * inv))
        mn, mx = np.fmin(a, b), np.fmax(a, b)  # fminf / fmaxf: a NaN operand yields the other one
        t0 = np.fmax(np.fmax(mn[:, 0], mn[:, 1]), np.fmax(mn[:, 2], F(0)))
        t1 = np.fmin(np.fmin(mx[:, 0], mx[:, 1]), mx[:, 2])
        return ~(t0 > t1 * F(1.00001) + F(1e-30)), t0


def ray_a(d):
    """a = 0.5f * k.a2 with a2 = 2.0f * sqlen(ray) (rfx_intersect.h ray_const), in float32."""
    with np.errstate(over="ignore", under="ignore"):
        sq = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        return F(0.5) * (F(2.0) * sq)


def prune(t0, a, best_sq, rng):
    """The walkers' prune: d0 = t0 * len, d0 * d0 > h.sq * 1.001f, with len = sqrt(a) inside [2^-100, 2^100], else 0."""
    with np.errstate(all="ignore"):
        ln = np.where((a >= F(2.0 ** -100)) & (a <= F(2.0 ** 100)), approx(np.sqrt(a), rng), F(0))
        d0 = t0 * ln
        return d0 * d0 > best_sq * F(1.001)


def prune_before(t0, a, best_sq):
    """The expression the walkers had: t0 * t0 * a > h.sq * 1.001f."""
    with np.errstate(all="ignore"):
        return t0 * t0 * a > best_sq * F(1.001)


def layers_boxes(L):
    """Per (triangle, ray) the reference reports as hit on the `layers` rays of length L: the triangle's box, the
    ray, and the hit's squared distance."""
    desc = E.desc_of("layers")
    rays = E.layers_rays(L)
    _, tab = E.composed("layers", "L" + L)
    ti, ri = np.nonzero(tab[:, :, 0] > 0)
    v = np.array([ob[1:4] for ob in desc.objects], np.float64)  # (48, 3, 3)
    lo, hi = v.min(axis=1)[ti], v.max(axis=1)[ti]
    dist = tab[ti, ri, 10]
    return lo, hi, rays[ri], (dist * dist).astype(F)


def tree_margins(lo, hi, ref):
    """mt of a box as rfx_scene.cpp computes it: (|centre - ref| + half-diagonal) * 1.0001, rounded up."""
    c, h = (lo + hi) * 0.5, (hi - lo) * 0.5
    mt = (np.linalg.norm(c - ref, axis=1) + np.linalg.norm(h, axis=1)) * 1.0001
    return np.nextafter(mt.astype(F), F(np.inf))


@pytest.mark.parametrize("L", E.LAYERS_LENGTHS)
def test_layers_hits_are_never_pruned(L):
    """Every triangle the reference reports as hit has its own box kept by the box test, and not pruned while the
    best squared distance is at least the triangle's own (taken 2^-20 below the reference's distance squared: the
    slack of one rounding of the square against the device's |ray t|^2).  An enclosing node's box is entered no
    later, so it is kept too."""
    rng = np.random.default_rng(20261020)
    lo, hi, rays, sq = layers_boxes(L)
    assert len(sq) >= 24 * E.LAYERS_N * 3 // 4
    ref = np.zeros((len(sq), 3))
    mt = tree_margins(lo, hi, ref)
    k, t0 = slab(lo.astype(F), hi.astype(F), rays[:, 0:3], rays[:, 3:6], ref.astype(F), mt, rng)
    assert k.all(), (L, int((~k).sum()))
    a = ray_a(rays[:, 3:6])
    for best in (sq * F(1 - 2.0 ** -20), sq * F(4.0), np.full_like(sq, np.inf)):
        p = prune(t0, a, best, rng)
        assert not p.any(), (L, int(p.sum()), t0[p][:4].tolist(), a[p][:4].tolist(), best[p][:4].tolist())


def random_boxes(n, rng):
    """n boxes, each with a ray of any length that reports a hit at a point inside it: (lo, hi, o, d, ref, mt, the
    hit's squared distance), the rays whose hit parameter the reference accepts (t > 2^-63)."""
    size = np.exp(rng.uniform(np.log(1e-3), np.log(5.0), (n, 3)))          # half extents
    centre = rng.uniform(-20.0, 20.0, (n, 3))
    ref = centre + rng.uniform(-15.0, 15.0, (n, 3))
    q = centre + rng.uniform(-1.0, 1.0, (n, 3)) * size                      # the hit point
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    dist = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), n))
    o = (q - u * dist[:, None]).astype(F)
    length = np.exp(rng.uniform(np.log(VERY_SMALL), np.log(1e20), n))
    d = (u * length[:, None]).astype(F)
    # the hit as the reference computes it from the float32 ray: t, then |ray t|^2
    real = np.linalg.norm(q - o.astype(np.float64), axis=1)
    t = (real / np.linalg.norm(d.astype(np.float64), axis=1)).astype(F)
    with np.errstate(all="ignore"):
        p = d * t[:, None]
        sq = ((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]).astype(F)
    ok = (t > F(VERY_SMALL)) & np.isfinite(d).all(1) & (sq > F(1e-8))
    lo, hi = (centre - size).astype(F), (centre + size).astype(F)
    mt = tree_margins(centre - size, centre + size, ref)
    return [x[ok] for x in (lo, hi, o, d, ref.astype(F), mt, sq)]


def test_random_boxes_with_rays_of_every_length_are_never_pruned():
    rng = np.random.default_rng(20261021)
    lo, hi, o, d, ref, mt, sq = random_boxes(1 << 16, rng)
    assert len(sq) > (1 << 16) * 3 // 4
    length = np.linalg.norm(d.astype(np.float64), axis=1)
    assert (length < 1e-17).sum() > 500 and (length > 1.3e19).sum() > 500  # both ends are sampled
    k, t0 = slab(lo, hi, o, d, ref, mt, rng)
    assert k.all(), int((~k).sum())
    a = ray_a(d)
    p = prune(t0, a, sq * F(1 - 2.0 ** -20), rng)
    assert not p.any(), (int(p.sum()), length[p][:4].tolist(), t0[p][:4].tolist(), sq[p][:4].tolist())
    # the prune still works where it always did: for rays of moderate length a box entered twice as far away as the
    # best hit is skipped
    mid = (a >= F(2.0 ** -100)) & (a <= F(2.0 ** 100)) & (t0 > 0)
    with np.errstate(all="ignore"):
        entry = (t0.astype(np.float64) * length) ** 2
    far = prune(t0, a, (entry * 0.25).astype(F), rng)
    assert mid.sum() > 10000 and far[mid & (entry > 1e-30)].all()


def test_the_product_form_pruned_boxes_that_hold_the_closest_hit():
    """What this file guards against, shown on the same inputs: t0 * t0 * a prunes kept boxes of reported hits at
    |ray| = 1e-18 (t0 * t0 overflows) and at 3e19 (a is +inf) -- on `layers` nearly every one."""
    rng = np.random.default_rng(20261020)
    for L in ("1e-18", "3e19"):
        lo, hi, rays, sq = layers_boxes(L)
        ref = np.zeros((len(sq), 3))
        k, t0 = slab(lo.astype(F), hi.astype(F), rays[:, 0:3], rays[:, 3:6], ref.astype(F),
                     tree_margins(lo, hi, ref), rng)
        p = prune_before(t0, ray_a(rays[:, 3:6]), sq * F(4.0))
        assert p[k].mean() > 0.9, (L, float(p[k].mean()))
    lo, hi, rays, sq = layers_boxes("1")
    ref = np.zeros((len(sq), 3))
    k, t0 = slab(lo.astype(F), hi.astype(F), rays[:, 0:3], rays[:, 3:6], ref.astype(F), tree_margins(lo, hi, ref), rng)
    assert not prune_before(t0, ray_a(rays[:, 3:6]), sq * F(1 - 2.0 ** -20)).any()
