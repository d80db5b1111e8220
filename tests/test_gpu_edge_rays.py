"""Edge rays on the GPU: the ray batches, hit queries and ordered calls of rfx.h on rays no pinhole frame or reflection
produces (tests/edge_rays.py) -- zero and -0.0 components, directions from 3e-19 to 1e20 long, origins up to 1e7
away, NaN and infinite words among good lanes -- through every kernel instantiation of the queries, with and without
the triangle tree.  The library promises the reference's answer for every float32 ray ("its direction is used as
given", rfx.h), so the bar is bit equality on every word: the queries against hits_helpers.compose, the colours against
rays_helpers.oracle_trace.  tests/test_edge_rays_host.py asserts that the reference reports hits in every regime.

What each group guards, and how it fails if that is broken (tests/test_bvh_prune_bound.py replays the first on the CPU):
  * `layers` -- 24 candidates per ray, the winner never the lowest index -- against a walker's distance prune that
    fires on an overflowed product (t0 * t0 * |ray|^2 at |ray| = 1e-18 or 3e19): the walk then keeps the first
    triangle it meets, which on these rays is the winner only if the tree happens to be walked front to back;
  * `graze` against a reject before the division that takes nz^2 * 2 |ray|^2 = +inf for `beyond the best hit`: 56
    rays meet the farther of two crossings first in insertion order;
  * `far_1e7` on the small scenes and `far` on `layers` against a winner's record that is not written whole when the
    candidate takes inside tri_takes' 2^-20 band (rfx_intersect.h hit_take): the hit is then shaded with the record
    of another object -- a wrong normal, reflection and colour under the right object index;
  * `axis` against unclamped reciprocals in ray_inv (a NaN slab end culls boxes the ray passes through);
  * the containment case against a make_bundle that ignores `bad`: a NaN lane would then set the wave's cone, and the
    good lanes' objects be culled.
"""
import numpy as np
import pytest

import edge_rays as E
import oracle as orc
from hits_helpers import PLANES, any_hit, same_bits
from rays_helpers import SEED
from reflaxman_amd import _lib

pytestmark = pytest.mark.gpu

# (scene, tri_accel, the query kernel it must run: (small scene, planes, triangle tree)) -- test_gpu_hits.py's tree
# modes for these scenes, soup300 with the tree, and `layers` without a tree, with it, and with narrow bundles on it
CASES = [("default", None, (True, False, False)), ("planes", None, (True, True, False)),
         ("planes300", None, (False, True, False)), ("stress4096", None, (False, False, False)),
         ("soup300", None, None), ("soup300", 1, (False, False, True)),
         ("mesh40x32", None, None), ("mesh40x32", -1, (False, False, True)), ("mesh40x32", 2, (False, False, True)),
         ("mesh100_plane", 1, (False, True, True)),
         ("layers", 0, (False, False, False)), ("layers", 1, (False, False, True)), ("layers", 2, (False, False, True))]
assert len({c[2] for c in CASES if c[2]}) == 6  # all six instantiations (rfx_trace_hits.hip launch_query_hits)


def renderer(name, tri_accel=None, form=None):
    """Renderer with the scene uploaded (the Scene kept alive on it); form: the kernel the case is meant to run."""
    from reflaxman_amd.render import Renderer, build_scene
    desc = E.desc_of(name)
    s, cam = build_scene(desc)
    r = Renderer(sphere_seed=SEED, jitter_seed=77)
    if tri_accel is not None:
        r.set_tri_accel(tri_accel)
    r.set_scene(s)
    r._edge_scene = s
    info = r.accel_info()
    if form is not None:
        n_pln = sum(1 for ob in desc.objects if ob[0] == "plane")
        got = (desc.n_spheres <= 32 and desc.n_triangles <= 32, n_pln > 0, info.tri_nodes > 0)
        assert got == form, (name, tri_accel, got)
    if tri_accel == 2:
        assert info.narrow_tri_bvh
    if name == "layers":
        assert (info.tri_nodes > 0) == (tri_accel > 0)
    return r


def dev(a):
    import torch
    a = np.array(a)  # (a copy: the shared references are read-only)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def side_stream(fn):
    import torch
    with torch.cuda.stream(torch.cuda.Stream()):
        out = fn()
        torch.cuda.current_stream().synchronize()
    return out


def order_arg(order):
    return order if order is None or isinstance(order, str) else dev(np.asarray(order, np.uint32))


def hits(r, rays, raster_width=0, order=None):
    out = side_stream(lambda: r.query_hits(dev(rays), raster_width=raster_width, order=order_arg(order)))
    return {k: v.cpu().numpy() for k, v in out.items()}


def shadow(r, rays, skip=None, raster_width=0, order=None):
    out = side_stream(lambda: r.occluded(dev(rays), None if skip is None else dev(np.asarray(skip, np.int32)),
                                         raster_width=raster_width, order=order_arg(order)))
    return out.cpu().numpy()


def trace(r, rays, depth, **kw):
    if "order" in kw:
        kw["order"] = order_arg(kw["order"])
    out = side_stream(lambda: r.trace_rays(dev(rays), depth, **kw))
    r.synchronize()  # (the pre-pass's error word)
    return out.cpu().numpy()


def fixed_permutation(n):
    return np.random.default_rng(12).permutation(n).astype(np.uint32)


def plane_diffs(got, want, rays, tag, sel=None):
    """One line per plane that differs in any bit (on the rays `sel`): the first rays, their words, and the ray."""
    out = []
    for k in want:
        g, w = (got[k], want[k]) if sel is None else (got[k][sel], want[k][sel])
        bad = same_bits(g, w)
        if bad.size:
            i = int(bad[0] if sel is None else np.flatnonzero(sel)[bad[0]])
            out.append((tag, k, int(bad.size), bad[:6].tolist(), g[bad[0]].tolist(), w[bad[0]].tolist(), rays[i].tolist()))
    return out


def report(diffs):
    """The assertion message: how many comparisons differ, and the first of them in full, one per line."""
    return "%d differ:\n" % len(diffs) + "\n".join(repr(d) for d in diffs[:8])


def flag_diffs(got, want, tag):
    bad = np.flatnonzero(got != want)
    return [(tag, "occluded", int(bad.size), bad[:6].tolist(), got[bad[:2]].tolist(), want[bad[:2]].tolist())] \
        if bad.size else []


# ------------------------------------------------------------------ hit queries
@pytest.mark.parametrize("name,tri_accel,form", CASES)
def test_queries_equal_the_composed_reference(name, tri_accel, form):
    """Every family, `mixed` and both rotations of `nonfinite` (on `layers`: its five lengths, `graze` and `far`), as a linear
    batch and as rasters 21 and 24 wide: all six planes, the any-hit with nothing left out, and with each ray leaving
    out its own winner.  (Not `occluded == (object >= 0)`: a hit at infinite distance occludes and never wins.)"""
    r = renderer(name, tri_accel, form)
    diffs = []
    for fam in E.batches(name):
        rays = E.batch(name, fam)
        want, tab = E.composed(name, fam)
        occ, own = any_hit(tab), any_hit(tab, want["object"])
        for rw in (0, 21, 24):
            tag = (name, tri_accel, fam, rw)
            got = hits(r, rays, raster_width=rw)
            assert sorted(got) == sorted(PLANES)
            diffs += plane_diffs(got, want, rays, tag)
            diffs += flag_diffs(shadow(r, rays, raster_width=rw), occ, tag + ("no skip",))
            diffs += flag_diffs(shadow(r, rays, want["object"], raster_width=rw), own, tag + ("own winner",))
    r.close()
    assert not diffs, report(diffs)


@pytest.mark.parametrize("name,tri_accel,form", CASES)
def test_ordered_queries_equal_the_unordered_ones(name, tri_accel, form):
    """`mixed` and both rotations of `nonfinite` (on `layers`: a short, a long, the grazing and the far batch) under the
    library's coherent order and under a fixed random permutation: word for word the unordered call's answers."""
    r = renderer(name, tri_accel, form)
    diffs = []
    for fam in (("L1e-18", "L3e19", "graze", "far") if name == "layers" else ("mixed", "nonfinite", "nonfinite_rot")):
        rays = E.batch(name, fam)
        plain = hits(r, rays)
        winner = plain["object"]
        occ, own = shadow(r, rays), shadow(r, rays, winner)
        for tag, order in (("coherent", "coherent"), ("random", fixed_permutation(len(rays)))):
            t = (name, tri_accel, fam, tag)
            diffs += plane_diffs(hits(r, rays, order=order), plain, rays, t)
            diffs += flag_diffs(shadow(r, rays, order=order), occ, t + ("no skip",))
            diffs += flag_diffs(shadow(r, rays, winner, order=order), own, t + ("own winner",))
    r.close()
    assert not diffs, report(diffs)


# ------------------------------------------------------------------ containment
@pytest.mark.parametrize("name,tri_accel", [("default", None), ("planes300", None), ("stress4096", None),
                                            ("mesh40x32", 2), ("layers", 1)])
def test_a_bad_lane_changes_no_good_lane(name, tri_accel):
    """A `nonfinite` batch whose good lanes are the unchanged base rays: their outputs are those of the plain base
    batch, with a bad ray as wave 0's first lane (the bundle's reference lane) and rotated so that it is not.  Device
    against device: a failure here names the wave-wide state (the bundle, the culls) and not the reference."""
    from rays_helpers import incoherent_rays
    base = E.layers_rays("1") if name == "layers" else incoherent_rays(E.RAYS_OF.get(name, name))
    n = len(base)
    r = renderer(name, tri_accel)
    diffs = []
    for rot in (0, E.NONFINITE_ROTATION):
        roll = lambda a: np.roll(a, -rot, axis=0)
        rays, good = roll(E.nonfinite_of(base)), roll(~E.nonfinite_edited(n))
        plain_rays = roll(base)
        assert np.array_equal(rays[good], plain_rays[good]) and good[0] == bool(rot) and n // 5 <= (~good).sum() <= n // 4
        for rw in (0, 24):
            tag = (name, rot, rw)
            want = hits(r, plain_rays, raster_width=rw)
            got = hits(r, rays, raster_width=rw)
            diffs += plane_diffs(got, want, rays, tag, sel=good)
            winner = want["object"]
            for skip in (None, winner):
                a = shadow(r, rays, skip, raster_width=rw)
                b = shadow(r, plain_rays, skip, raster_width=rw)
                diffs += flag_diffs(a[good], b[good], tag + ("skip" if skip is not None else "no skip",))
    r.close()
    assert not diffs, report(diffs)


# ------------------------------------------------------------------ colours
COLOUR_CASES = [("default", None), ("planes300", None), ("soup300", 1), ("stress4096", None), ("layers", 0),
                ("layers", 1)]
# the oracle's counters a ray batch's stats kernel must reproduce: what happened to every ray and segment
OUTCOMES = ("rays", "segments", "hit_sph", "hit_tri", "hit_pln", "sky", "dielectric", "metal", "continue")


@pytest.mark.parametrize("name,tri_accel", COLOUR_CASES)
def test_colours_equal_the_per_ray_oracle(name, tri_accel):
    """rfx_trace_rays at depths 1 and 8 on the batches the 1 x 1 oracle can carry (len_1e-18, len_1e19, len_3e19,
    axis_pos, far_1e3, far_1e7 and the finite, -0.0-free part of mixed; on `layers` four lengths, `graze`, `far`): linear, raster 24,
    in coherent order, and as the counting form -- the oracle's colours, its stream's end state, its outcome counters."""
    import torch
    r = renderer(name, tri_accel)
    diffs = []

    def check(got, want, rays, tag):
        bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))
        if bad.size:
            diffs.append((tag, int(bad.size), bad[:6].tolist(), got[bad[0]].tolist(), want[bad[0]].tolist(),
                          rays[bad[0]].tolist()))

    for fam in E.colour_batches(name):
        rays = E.colour_rays(name, fam)
        for depth in (1, 8):
            want, end, ocnt = E.colours(name, fam, depth, SEED)
            for tag, kw in (("linear", {}), ("raster24", {"raster_width": 24}), ("coherent", {"order": "coherent"})):
                r.set_rng(SEED, 77)
                check(trace(r, rays, depth, **kw), want, rays, (name, tri_accel, fam, depth, tag))
                if r.get_rng() != (end, 77):
                    diffs.append((name, fam, depth, tag, "stream", r.get_rng(), end))
            r.set_rng(SEED, 77)
            cnt = torch.zeros(_lib.RFX_NCOUNTERS, dtype=torch.int64, device="cuda")
            check(trace(r, rays, depth, counters=cnt), want, rays, (name, tri_accel, fam, depth, "counting"))
            gc = cnt.cpu().numpy().view(np.uint64)
            for k in OUTCOMES:
                i = list(orc.COUNTER_NAMES).index(k)
                if int(gc[i]) != int(ocnt[i]):
                    diffs.append((name, fam, depth, "counter", k, int(gc[i]), int(ocnt[i])))
    r.close()
    assert not diffs, report(diffs)
