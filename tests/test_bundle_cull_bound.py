"""The wave-bundle culls (rfx_bundle.h) drop no object the reference reports as hit by a ray of the bundle.

The replay is tests/bundle_cull.py: make_bundle / make_bundle_ball / make_bundle_quad, the cone term of cull_chunk and
cull_small, cull_small's plane rule (`away`) and tri_footprint_misses in float32, on the library's own records
(rfx_scene_cull_dump).  The verdict is the reference's: oracle.kat("triangle" | "sphere"), a ray reported if its hit
flag or its any-hit flag is set.  2^14 bundles of 64 rays per family (aimed, departing, each also with spread origins,
a light's ball, a pixel's quadrilateral, spheres), each bundle on its own target and on its neighbour in the scene of
32; the footprint also on all 32 triangles of the aimed and quad bundles' scenes.

Asserted: no bundle carries a reported hit on an object a term drops (per term, per cond class [3, 100), [100, 300),
>= 300); records of cond >= 300 are inert (r = inf, zero normal), footprint records of cond >= 100 are (inf norms);
the non-vacuity shares below; every used margin fraction < 1 (the kernel's own margin, nothing tighter).

Measured (printed by the tests; the used fraction of the kernel's own margin by a bundle that carries a reported hit,
1 = dropped): away 0.84 (departing_spread; departing 0.60, aimed 0.48, aimed_spread 0.48, ball 0.49, quad 0.49,
surface 0.41); footprint 0.53 (aimed), 0.56 (quad); cone 0.00 in every family (make_bundle's own 4e-6 on the cosine
widens the cone by >= 2.8e-3 rad, so no carrier reaches the limit even without kCullRel).  Single rays: 0 reported
rays leave the plane in exact terms; in the record's float32 terms 128 do, by at most 2.2e-5 of |o - c| + r (0.022 of
the 1e-3 margin).  Shares: aimed 55% carriers; departing 12.0% dropped by away, 4.2% carriers; the footprint drops
12.6% (aimed) and 12.5% (quad) of the cond < 100 pairs the cone and the plane keep.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import bundle_cull as bc
from bundle_cull import F

N = 1 << 14
ALL = np.ones((N, 64), bool)


def pair(x):
    """(target, neighbour in the scene of 32) of per-object rows"""
    return np.stack([x, x[np.arange(len(x)) ^ 1]], axis=1)


@functools.lru_cache(maxsize=None)
def tris():
    G = bc.triangles(N, 20261021)
    G.recs, G.foot, _ = bc.library_records(V=G.V)
    G.cls = bc.cond_class(G.cond)
    for a in (G.V, G.recs, G.foot, G.cond, G.cls):
        a.setflags(write=False)
    return G


@functools.lru_cache(maxsize=None)
def spheres():
    rng = np.random.default_rng(20261022)
    S = SimpleNamespace(c=rng.uniform(-30.0, 30.0, (N, 3)).astype(F).astype(np.float64),
                        r=np.exp(rng.uniform(np.log(0.02), np.log(30.0), N)).astype(F).astype(np.float64))
    _, _, S.recs = bc.library_records(spheres=np.concatenate([S.c, S.r[:, None]], axis=1))
    return S


def verdicts(o, d, V, every=1):
    """any lane reported on (target, neighbour): (N, 2) bool; the neighbour's only for every `every`-th bundle (else
    False, with `known` False).  o, d: (N, 64[, k], 3)"""
    o = np.broadcast_to(o.reshape(N, 64, -1, 3) if o.ndim == 4 else o[:, :, None, :], d.reshape(N, 64, -1, 3).shape)
    o, d = o.reshape(N, -1, 3), d.reshape(N, -1, 3)
    hit = np.zeros((N, 2), bool)
    known = np.ones((N, 2), bool)
    hit[:, 0] = bc.reported_tri(o, d, V).any(1)
    sel = np.arange(N) % every == 0
    known[~sel, 1] = False
    hit[sel, 1] = bc.reported_tri(o[sel], d[sel], V[np.arange(N) ^ 1][sel]).any(1)
    return hit, known


@functools.lru_cache(maxsize=None)
def family(name):
    """bundles, replay and verdicts of a triangle family, computed once: o, d, B, T (terms on (target, neighbour)),
    hit, known (N, 2)"""
    G = tris()
    seed = {"aimed": 1, "departing": 2, "aimed_spread": 3, "departing_spread": 4, "ball": 5, "quad": 6}[name]
    rng = np.random.default_rng(100 + seed)
    X = SimpleNamespace(name=name)
    if name.startswith("departing"):
        X.o, X.d = bc.departing(G, seed, spread=name.endswith("spread"))
    else:
        p, out = bc.tri_silhouette(G, 50 + seed)
        X.o, X.d = bc.aimed(p, out, G.nrm, G.size, seed, spread=name in ("aimed_spread", "ball"))
    if name == "ball":
        # shadow rays toward a light beyond the target: the origins are the spread bundle's, the light lies on the axis
        # ray 1.2 .. 5 times as far as the aim point, R / |d| in 1e-3 .. 0.6 (both sides of the sb < 0.5 cut-off)
        k = np.exp(rng.uniform(np.log(1.2), np.log(5.0), N))
        light = (X.o[:, 0].astype(np.float64) + X.d[:, 0].astype(np.float64) * k[:, None]).astype(F)
        X.d = light[:, None, :] - X.o
        X.R = (np.linalg.norm(X.d[:, 0].astype(np.float64), axis=1) *
               np.exp(rng.uniform(np.log(1e-3), np.log(0.6), N))).astype(F)
        X.B = bc.make_bundle_ball(X.o, X.d, X.R, ALL, rng)
        X.rays = bc.shadow_rays(X.o, X.d, X.R, bc.ball_samples())
        X.hit, X.known = verdicts(X.o, X.rays, G.V, every=4)
    elif name == "quad":
        s1 = (X.d[:, 1].astype(np.float64) - X.d[:, 0]), (X.d[:, 8].astype(np.float64) - X.d[:, 0])
        X.dq = bc.quad_corners(X.d, *s1)
        X.B = bc.make_bundle_quad(X.o, X.dq, ALL, rng)
        X.rays = bc.quad_rays(X.dq)
        X.hit, X.known = verdicts(X.o, X.rays, G.V, every=4)
    else:
        X.B = bc.make_bundle(X.o, X.d, ALL, rng)
        X.hit, X.known = verdicts(X.o, X.d, G.V)
    X.T = bc.cull_terms(pair(G.recs), X.B, rng)
    X.cls = pair(G.cls)
    return X


def used_away(T):
    """the fraction of `away`'s margins a (bundle, triangle) uses: both |side| / ms and |an| / ma pass 1 on the same
    side when it drops"""
    with np.errstate(invalid="ignore", divide="ignore"):
        same = np.sign(T.side) * np.sign(T.an) > 0
        return np.where(same, np.fmin(np.abs(T.side) / T.ms, np.abs(T.an) / T.ma), F(0))


def used_cone(rec, B, T, rng):
    """the fraction of the kCullRel widening the cone term uses: (lim0 - va) / (lim0 - lim), lim0 the limit without
    kCullRel; 1 is a drop"""
    T0 = bc.cull_terms(rec, B, rng, k_rel=0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        u = (T0.lim - T.va) / (T0.lim - T.lim)
    return np.where((T.L > T.rp) & np.isfinite(u), u, F(0))


def audit(X, recs):
    """the per-term, per-class drop counts of a family, and its worst used fractions among hit carriers"""
    ok = X.B.ok[:, None]
    carried = X.hit & X.known
    out = {}
    for term in ("cone", "away"):
        drop = getattr(X.T, term) & ok
        for k in range(3):
            out[term, k] = int((drop & carried & (X.cls == k)).sum())
        out[term, "dropped"] = int((drop & X.known).sum())
    rng = np.random.default_rng(9)
    out["used_away"] = float(used_away(X.T)[carried & ok].max(initial=0.0))
    out["used_cone"] = float(used_cone(recs, X.B, X.T, rng)[carried & ok].max(initial=0.0))
    out["ok"] = float(X.B.ok.mean())
    out["carry"] = float(X.hit[:, 0].mean())
    return out


TRI_FAMILIES = ["aimed", "departing", "aimed_spread", "departing_spread", "ball", "quad"]


def test_records_of_ill_conditioned_triangles_are_inert():
    G = tris()
    near = lambda c: np.abs(G.cond / c - 1.0) < 1e-2       # the library's float cond may class these the other way
    bad = (G.cond >= 300.0) & ~near(300.0)
    assert bad.sum() > N // 20
    assert np.isposinf(G.recs[bad, 3]).all() and (G.recs[bad, 4:8] == 0).all()
    nofoot = (G.cond >= 100.0) & ~near(100.0)
    assert nofoot.sum() > N // 10
    assert np.isposinf(G.foot[nofoot][:, [3, 7, 11]]).all()
    # and the other records do cull: finite radius, unit normal, finite footprint (a tiny triangle whose determinant
    # the reference treats as zero is inert at any cond)
    good = (G.cond < 300.0) & ~near(300.0)
    live = np.isfinite(G.recs[:, 3]) & (np.abs(np.linalg.norm(G.recs[:, 4:7], axis=1) - 1.0) < 1e-6)
    foot = np.isfinite(G.foot[:, [3, 7, 11]]).all(1)
    print(f"records: {int(live[good].sum())} of {int(good.sum())} cond < 300 cull; "
          f"{int(foot[(G.cond < 100) & ~near(100.0)].sum())} of {int(((G.cond < 100) & ~near(100.0)).sum())} cond < 100 "
          f"have a footprint")
    assert live[good].mean() > 0.9 and foot[(G.cond < 100.0) & ~near(100.0)].mean() > 0.9
    assert not live[bad].any() and not foot[nofoot].any()


@pytest.mark.parametrize("name", TRI_FAMILIES)
def test_no_term_drops_a_triangle_a_ray_of_the_bundle_is_reported_on(name):
    X = family(name)
    a = audit(X, pair(tris().recs))
    print(f"{name}: B.ok {a['ok']:.3f}, carriers {a['carry']:.3f}, dropped cone {a['cone', 'dropped']} away "
          f"{a['away', 'dropped']} of {int(X.known.sum())} pairs; worst used: away {a['used_away']:.3f} "
          f"cone {a['used_cone']:.3f}")
    for term in ("cone", "away"):
        for k in range(3):
            assert a[term, k] == 0, (name, term, bc.CLASSES[k], a[term, k])
    assert a["used_away"] < 1.0 and a["used_cone"] < 1.0
    # non-vacuity: the bound is usable, the terms do drop neighbours, every class carries reported hits
    assert a["ok"] > (0.25 if name == "ball" else 0.9)
    assert a["cone", "dropped"] > X.known[:, 1].sum() // 4
    carried = X.hit[:, 0]
    for k in range(3):
        assert (carried & (X.cls[:, 0] == k)).sum() > carried.sum() // 100, (name, bc.CLASSES[k])


def test_aimed_bundles_carry_reported_hits():
    assert family("aimed").hit[:, 0].mean() >= 1 / 3


def test_departing_bundles_are_dropped_and_still_carry_hits():
    X = family("departing")
    tree = X.cls[:, 0] < 2
    away = X.T.away[:, 0] & X.B.ok
    print(f"departing: away drops {away[tree].mean():.3f} of the cond < 300 bundles, {X.hit[:, 0].mean():.3f} carry a hit")
    assert away[tree].mean() >= 1 / 16
    assert X.hit[:, 0].mean() >= 1 / 64


def test_bundles_leaving_a_triangle_s_own_surface():
    """4 x 2^14 bundles from points on the triangles themselves (bundle_cull.surface): the record's side is float
    rounding there, and the reference reports the crossing at t ~ 0 whenever its own rounding puts it ahead"""
    G = tris()
    worst, viol, dropped, carried = 0.0, 0, 0, 0
    for seed in range(4):
        rng = np.random.default_rng(40 + seed)
        o, d = bc.surface(G, seed)
        hit = bc.reported_tri(o, d, G.V).any(1)
        B = bc.make_bundle(o, d, ALL, rng)
        T = bc.cull_terms(G.recs[:, None, :], B, rng)
        drop = (T.away | T.cone)[:, 0] & B.ok
        viol, dropped, carried = viol + int((drop & hit).sum()), dropped + int(drop.sum()), carried + int(hit.sum())
        worst = max(worst, float(used_away(T)[:, 0][hit & B.ok].max(initial=0.0)))
    print(f"surface: {carried} carriers of {4 * N}, {dropped} dropped; worst used fraction of away's margins {worst:.3f}")
    assert viol == 0
    assert worst < 1.0
    assert carried >= 4 * N // 8


def test_ball_bundles_cover_both_sides_of_the_cut_off():
    X = family("ball")
    sbm = X.B.sb.max(1)
    assert (sbm < 0.5).mean() > 0.25 and (sbm >= 0.5).mean() > 0.02
    assert not X.B.ok[sbm >= 0.5].any()
    assert X.hit[:, 0].mean() >= 1 / 3


@pytest.mark.parametrize("name", ["aimed", "quad"])
def test_footprint_drops_no_reported_triangle(name):
    """the footprint on all 32 triangles of each bundle's scene; verdicts for the pairs it decides (those the cone
    and the plane keep)"""
    G, X = tris(), family(name)
    rng = np.random.default_rng(77)
    blk = (np.arange(N) // 32 * 32)[:, None] + np.arange(32)[None, :]          # (N, 32) triangle indices
    T = bc.cull_terms(G.recs[blk], X.B, rng)
    miss, used = bc.tri_footprint_misses(G.foot[blk], T.side, T.an, X.B, rng)
    cls = G.cls[blk]
    decides = ~T.cone & ~T.away & X.B.ok[:, None] & np.isfinite(G.foot[blk][..., 3])
    bi, ti = np.nonzero(decides)
    rays = X.rays if name == "quad" else X.d[:, :, None, :]
    ro = np.broadcast_to(X.o[:, :, None, :], rays.shape).reshape(N, -1, 3)
    hit = np.zeros(decides.shape, bool)
    hit[bi, ti] = bc.reported_tri(ro[bi], rays.reshape(N, -1, 3)[bi], G.V[blk[bi, ti]]).any(1)
    share = (miss & decides)[cls == 0].sum() / max(1, decides[cls == 0].sum())
    worst = float(used[hit & decides].max(initial=0.0))
    print(f"footprint ({name}): decides {int(decides.sum())} pairs, drops {share:.4f} of the cond < 100 ones, "
          f"{int((hit & decides).sum())} carry a reported hit; worst used fraction {worst:.3f}")
    for k in range(3):
        assert not (miss & decides & hit & (cls == k)).any(), (name, bc.CLASSES[k])
    assert not (miss & (cls > 0) & ~np.isclose(G.cond[blk], 100.0, rtol=1e-2)).any()   # gated at cond < 100
    assert worst < 1.0
    assert share >= 1 / 8
    assert (hit & decides & (cls == 0)).sum() > N // 8


@pytest.mark.parametrize("spread", [False, True])
def test_cone_term_keeps_every_reported_sphere(spread):
    """spheres through cull_chunk / cull_small: the cone term with the bundle's own widening"""
    S = spheres()
    rng = np.random.default_rng(31 + spread)
    o, d = bc.aimed_sphere(S.c, S.r, 8 + spread, spread=spread)
    B = bc.make_bundle(o, d, ALL, rng)
    recs = pair(S.recs)
    T = bc.cull_terms(recs, B, rng)
    nb = np.arange(N) ^ 1
    hit = np.stack([bc.reported_sph(o, d, S.c, S.r).any(1), bc.reported_sph(o, d, S.c[nb], S.r[nb]).any(1)], axis=1)
    drop = (T.cone | ~bc.cull_chunk(recs[..., :4], B, rng)) & B.ok[:, None]    # cull_small's and cull_chunk's
    assert not T.away.any()                                                     # a sphere's record has no plane
    worst = float(used_cone(recs, B, T, rng)[hit & B.ok[:, None]].max(initial=0.0))
    print(f"spheres (spread {spread}): B.ok {B.ok.mean():.3f}, carriers {hit[:, 0].mean():.3f}, neighbours dropped "
          f"{drop[:, 1].mean():.3f}; worst used fraction of kCullRel {worst:.3f}")
    assert not (drop & hit).any(), int((drop & hit).sum())
    assert worst < 1.0
    assert hit[:, 0].mean() >= 1 / 3 and drop[:, 1].mean() > 0.5 and B.ok.mean() > 0.9


def test_single_ray_rounding_behind_the_plane_rule():
    """The figure behind cull_small's "2e-4": a ray that starts on one side of the plane and leaves it is still
    reported by the reference while its height is under x (|o - centre| + r) or its direction's cosine to the normal
    under x.  The worst x over the reported rays of the aimed and departing families (cond < 300), in exact terms
    (float64 plane of the float vertices: the reference's own rounding) and in the cull's terms (the record's float32
    normal and offset at absolute coordinates: what the 1e-3 margins must cover)."""
    G = tris()
    rng = np.random.default_rng(5)
    worst = {"exact": 0.0, "record": 0.0}
    count = {"exact": 0, "record": 0}
    culls = np.isfinite(G.recs[:, 3])
    for name in ("aimed", "departing"):
        X = family(name)
        o, d = X.o.astype(np.float64), X.d.astype(np.float64)
        hit = bc.reported_tri(X.o, X.d, G.V) & culls[:, None]
        scale = np.linalg.norm(o - G.cen[:, None, :], axis=2) + G.rad[:, None]
        side = ((o - G.V[:, None, 0]) * G.nrm[:, None, :]).sum(2)
        an = (d * G.nrm[:, None, :]).sum(2) / np.linalg.norm(d, axis=2)
        rside = bc.cdot(G.recs[:, None, 4:7], X.o) - G.recs[:, None, 7]
        ran = bc.cdot(G.recs[:, None, 4:7], X.d * bc.rsq(bc.cdot(X.d, X.d), rng)[..., None])
        for key, s_, a_ in (("exact", side, an), ("record", rside.astype(np.float64), ran.astype(np.float64))):
            leaving = hit & (s_ * a_ > 0)
            x = np.minimum(np.abs(s_) / scale, np.abs(a_))
            worst[key] = max(worst[key], float(x[leaving].max(initial=0.0)))
            count[key] += int(leaving.sum())
    for key in worst:
        print(f"single rays ({key} terms): {count[key]} reported while leaving the plane; worst min(|side| / (|o - c| + r), "
              f"|cos|) = {worst[key]:.3e} ({worst[key] / 1e-3:.3f} of the 1e-3 margin)")
    assert count["record"] > 0
    assert worst["exact"] < 1e-3 and worst["record"] < 1e-3
