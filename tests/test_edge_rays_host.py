"""Edge rays, the part that needs no GPU: the conditions on the inputs of tests/test_gpu_edge_rays.py, asserted on the
reference alone.  A family that stopped reaching the regime it is named for -- no hits left at |ray| = 1e-18, say --
would let the GPU comparison pass on misses; the floors below sit under the numbers observed with the project's
oracle (given beside them)."""
import numpy as np
import pytest

import edge_rays as E
import oracle as orc
from hits_helpers import FLT_MAX, any_hit, kinds
from rays_helpers import NRAYS, SEED, incoherent_rays, oracle_trace

SCENES = ("default", "planes300", "soup300", "mesh40x32", "stress4096")


def won(name, fam):
    """[spheres, triangles, planes, misses] among the composed winners."""
    return kinds(E.desc_of(name), E.composed(name, fam)[0]["object"])


def test_the_families_are_what_they_are_named_for():
    name = "default"
    base = incoherent_rays(name)
    u = base[:, 3:6].astype(np.float64)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    for L in E.LENGTHS:
        r = E.family(name, "len_" + L)
        assert r.dtype == np.float32 and r.shape == (NRAYS, 6) and np.array_equal(r[:, 0:3], base[:, 0:3])
        assert np.allclose(np.linalg.norm(r[:, 3:6].astype(np.float64), axis=1), float(L), rtol=1e-6, atol=0)
    ax, ap = E.family(name, "axis"), E.family(name, "axis_pos")
    d = ax[:, 3:6]
    zero, neg = d == 0, (d == 0) & np.signbit(d)
    k = np.arange(NRAYS) % 7
    assert (zero.sum(1)[k < 3] == 1).all() and (zero.sum(1)[(k >= 3) & (k < 6)] == 2).all() and not zero[k == 6].any()
    assert not neg[k < 3].any() and (neg.sum(1)[(k >= 3) & (k < 6)] == 1).all()
    for c in range(3):
        assert zero[k == c, c].all() and neg[k == 3 + c, c].all() and zero[k == 3 + c, (c + 1) % 3].all()
    assert np.array_equal(ax, ap) and not np.signbit(ap[:, 3:6][ap[:, 3:6] == 0]).any()  # -0.0 == +0.0: the same values
    assert np.array_equal(ax[k == 6], base[k == 6])
    for D in E.FARS:
        r = E.family(name, "far_" + D)
        assert np.allclose(np.linalg.norm(r[:, 3:6].astype(np.float64), axis=1), 1.0, rtol=1e-6)
        back = r[:, 0:3].astype(np.float64) + u * float(D)
        assert np.abs(back - base[:, 0:3]).max() <= float(D) * 2.0 ** -22  # the same line, from D away
    nf, rot = E.family(name, "nonfinite"), E.family(name, "nonfinite_rot")
    edited = E.nonfinite_edited(NRAYS)
    assert edited[0] and not edited[E.NONFINITE_ROTATION] and not np.isfinite(nf[0]).all()
    assert np.array_equal(rot, nf[(np.arange(NRAYS) + E.NONFINITE_ROTATION) % NRAYS], equal_nan=True)
    assert np.array_equal(rot[0], base[E.NONFINITE_ROTATION])  # wave 0's reference lane is a good ray
    assert np.array_equal(nf[~edited], base[~edited]) and 70 <= edited.sum() <= 80
    bad = ~np.isfinite(nf)
    assert (bad.sum(1)[0::5] == 1).all() and bad.sum() == len(range(0, NRAYS, 5)) and bad.any(axis=0).all()
    assert np.isnan(nf).sum() >= 20 and (nf == np.inf).sum() >= 20 and (nf == -np.inf).sum() >= 20
    assert not nf[3::50, 3:6].any() and len(nf[3::50]) == 8
    mixed = E.family(name, "mixed")
    for i in range(NRAYS):
        assert np.array_equal(mixed[i], E.family(name, E.FAMILIES[i % len(E.FAMILIES)])[i], equal_nan=True)
    ok = E.oracle_ok(mixed)
    assert 330 <= ok.sum() < NRAYS and np.isfinite(mixed[ok]).all()


@pytest.mark.parametrize("L", E.LAYERS_LENGTHS)
def test_layers_every_ray_crosses_the_stack(L):
    """All 256 rays hit, the median ray hits 24 triangles, and no winner is the lowest-index triangle its ray hits:
    a walk that kept its first candidate, or the first in insertion order, would be wrong on every ray."""
    desc = E.desc_of("layers")
    assert len(desc.objects) == 48 and desc.n_triangles == 48
    want, tab = E.composed("layers", "L" + L)
    hit = tab[:, :, 0] > 0
    assert (want["object"] >= 0).all() and len(want["object"]) == E.LAYERS_N
    assert np.median(hit.sum(axis=0)) == 24
    assert (want["object"] != np.argmax(hit, axis=0)).all()
    # the winners are the outermost quads: the four triangles at z = -6 and z = 5.5, wherever they were inserted
    tris, order = E.layers_triangles()
    assert set(order[want["object"]].tolist()) == {0, 1, 46, 47}


def test_layers_grazing_rays():
    """`graze`: 2 |ray|^2 is +inf, (normal . ray)^2 is finite, at least 100 rays cross two quads and on at least 50 the
    nearer crossing has the higher index (observed: 114 and 56)."""
    rays = E.layers_graze()
    d = rays[:, 3:6]
    with np.errstate(over="ignore"):
        a = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        assert np.isfinite(a).all() and np.isinf(np.float32(2) * a).all() and np.isfinite(d[:, 2] * d[:, 2]).all()
    want, tab = E.composed("layers", "graze")
    hit = tab[:, :, 0] > 0
    assert (want["object"] >= 0).sum() >= 250
    assert (hit.sum(axis=0) >= 2).sum() >= 100
    assert ((want["object"] >= 0) & (want["object"] != np.argmax(hit, axis=0))).sum() >= 50


def in_band(tab):
    """Per ray: do two of the objects it hits lie within 2^-21 of each other in distance (2^-20 in the square)?"""
    with np.errstate(invalid="ignore"):
        d = np.where(tab[:, :, 0] > 0, tab[:, :, 10].astype(np.float64), np.inf)
    d = np.sort(d, axis=0)
    with np.errstate(invalid="ignore"):
        return (np.isfinite(d[1:]) & (d[1:] - d[:-1] <= d[:-1] * 2.0 ** -21)).any(axis=0)


def test_far_rays_decide_inside_the_band():
    """From 1e7 away the candidates of a ray lie inside the closest-hit rule's 2^-20 band: on `layers` for at least
    250 of the 256 rays, with the winner never the lowest index hit; on the small scenes `default` and `planes` at
    least 8 rays each are won by a triangle with a sphere hit inside the band behind it (observed 10 and 6 -- the rays
    on which a stale Hit::i showed)."""
    want, tab = E.composed("layers", "far")
    hit = tab[:, :, 0] > 0
    assert (want["object"] >= 0).sum() >= 250 and in_band(tab).sum() >= 250
    assert (np.median(hit.sum(axis=0)) >= 20) and (want["object"] != np.argmax(hit, axis=0)).sum() >= 200
    for name, floor in (("default", 8), ("planes", 5)):
        desc = E.desc_of(name)
        want, tab = E.composed(name, "far_1e7")
        kind = np.array([ob[0] for ob in desc.objects])
        tri = (want["object"] >= 0) & (kind[np.maximum(want["object"], 0)] == "triangle")
        sph_behind = ((tab[:, :, 0] > 0) & (kind == "sphere")[:, None]).any(axis=0)
        assert (tri & sph_behind & in_band(tab)).sum() >= floor, (name, int((tri & sph_behind & in_band(tab)).sum()))


# (family, scene): the least number of winners that are [spheres, triangles, planes, misses]; observed beside them
FLOORS = [
    ("len_1e-18", "soup300", [0, 100, 0, 0]),      # 121 triangle hits
    ("len_1e-18", "mesh40x32", [0, 100, 0, 0]),    # 107
    ("len_1e-18", "default", [0, 100, 0, 0]),      # 107
    ("len_1e-18", "planes300", [0, 100, 80, 0]),   # 125, plus 95 plane hits
    ("len_1e-18", "stress4096", [0, 100, 0, 0]),   # 125
    ("len_3e19", "soup300", [0, 60, 0, 0]),        # 77
    ("len_3e19", "mesh40x32", [0, 20, 0, 0]),      # 25
    ("len_3e19", "default", [0, 25, 0, 0]),        # 34
    ("len_3e19", "planes300", [0, 10, 150, 0]),    # 13, plus 173 plane hits
    ("len_1e20", "planes300", [0, 0, 100, 0]),     # 151 plane hits
    ("len_1e-9", "stress4096", [150, 0, 0, 0]),    # 176 sphere hits
    ("len_1e17", "stress4096", [150, 0, 0, 0]),    # 176
    ("far_1e5", "stress4096", [340, 0, 0, 0]),     # 357: the reference's own cancellation
    ("far_1e5", "default", [340, 0, 0, 0]),        # 345
    ("far_1e5", "mesh40x32", [340, 0, 0, 0]),      # 349
    ("far_1e5", "soup300", [0, 250, 0, 0]),        # 259
]


@pytest.mark.parametrize("fam,name,floor", FLOORS)
def test_the_reference_reports_hits_in_every_regime(fam, name, floor):
    got = won(name, fam)
    assert all(g >= f for g, f in zip(got, floor)), (fam, name, got)


def test_spheres_miss_where_the_reference_says_so():
    """|ray|^2 <= 2^-63 (1e-18, 3e-19) and 2 |ray|^2 = +inf (3e19, 1e20): no sphere is ever the winner."""
    for fam in ("len_1e-18", "len_3e-19", "len_3e19", "len_1e20"):
        for name in ("default", "planes300", "stress4096"):
            assert won(name, fam)[0] == 0, (fam, name)


@pytest.mark.parametrize("name", SCENES)
def test_axis_rays_hit_and_miss(name):
    got = won(name, "axis")
    assert sum(got[:3]) >= 60 and got[3] >= 100, (name, got)
    assert got == won(name, "axis_pos")


def test_a_hit_at_infinite_distance_occludes_but_never_wins():
    """`nonfinite` on planes300: at least 10 rays (observed 18) whose any-hit is 1 while the closest hit is a miss --
    a distance of +inf is never `< FLT_MAX`.  So no edge-ray test may assert occluded == (object >= 0)."""
    for fam in ("nonfinite", "nonfinite_rot"):
        want, tab = E.composed("planes300", fam)
        assert ((any_hit(tab) == 1) & (want["object"] < 0)).sum() >= 10, fam


@pytest.mark.parametrize("name", SCENES + ("planes", "mesh100_plane", "layers"))
def test_every_reference_word_is_finite(name):
    """Bit comparison is well defined: every word of every plane of the composed reference is finite, for every batch;
    and no object reports a hit at a NaN distance, which np.argmin -- unlike the reference's `<` -- would let win."""
    own = []
    for fam in E.batches(name):
        want, tab = E.composed(name, fam)
        for k, v in want.items():
            assert np.isfinite(v).all(), (name, fam, k)
        assert not np.isnan(tab[:, :, 10][tab[:, :, 0] > 0]).any(), (name, fam)
        miss = want["object"] < 0
        assert (want["distance"][miss] == FLT_MAX).all() and (want["distance"][~miss] < FLT_MAX).all()
        own.append(any_hit(tab, want["object"]))
    # each ray leaving out its own winner: over the batches, both answers occur often
    own = np.concatenate(own)
    assert (own == 1).sum() >= 100 and (own == 0).sum() >= 100, name


@pytest.mark.parametrize("name", ["default", "planes300", "soup300", "stress4096", "layers"])
def test_the_two_references_agree(name):
    """For every batch the 1 x 1 oracle can carry, the composed winners' kinds are the hit counters of a depth-1
    oracle_trace on the same rays."""
    for fam in E.colour_batches(name) + (() if name == "layers" else ("far_1e5",)):
        rays = E.batch(name, fam)
        ok = E.oracle_ok(rays)
        want, _ = E.composed(name, fam)
        got = kinds(E.desc_of(name), want["object"][ok])
        cnt = np.zeros(len(orc.COUNTER_NAMES), np.uint64)
        oracle_trace(E.desc_of(name), rays[ok], 1, SEED, cnt)
        c = {k: int(cnt[i]) for i, k in enumerate(orc.COUNTER_NAMES)}
        assert got == [c["hit_sph"], c["hit_tri"], c["hit_pln"], c["sky"]], (name, fam, got)
        assert c["rays"] == int(ok.sum())
