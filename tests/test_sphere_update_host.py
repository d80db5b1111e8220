"""Moving spheres, the host side (rfx.h "Moving spheres"; no device): rfx_scene_set_spheres against a scene built at the
same spheres, the host refit against the builder's own boxes, and the soundness of the refitted boxes and chunk bounds --
containment, and the float32 replay of the kernel's box test against the reference's verdicts (oracle.kat("sphere"))."""
import numpy as np
import pytest

from mesh_update import kept_prewide
from reflaxman_amd import _lib, scenes
from reflaxman_amd.render import build_scene
from sphere_update import (F, INFINITE_CENTRE, INFINITE_RADIUS, SEED, clamped, jiggle, moved_desc, record_words,
                           ref_point, shuffle, special_spheres, sph_data, sphere_boxes, tree_paths)

SCENES = {"stress33": lambda: scenes.stress_scene(33), "stress100": lambda: scenes.stress_scene(100),
          "soup1500s300": lambda: scenes.soup_scene(1500, n_spheres=300)}
_BUILT = {}


def built(key):
    """(description, Scene, dump) of a case, built once and never edited"""
    if key not in _BUILT:
        desc = SCENES[key]()
        s, _ = build_scene(desc)
        _BUILT[key] = (desc, s, s.sph_bvh_dump())
    return _BUILT[key]


# ------------------------------------------------------------------------------------------------ self-consistency
@pytest.mark.parametrize("key", list(SCENES))
def test_refit_to_the_scene_s_own_spheres_is_the_dump(key):
    desc, s, d = built(key)
    S = sph_data(desc)
    n = len(S)
    assert d["nodes"] > 0 and d["leaves"] == d["nodes"] + 1 == (n + 7) // 8 and d["leaf_size"] == 8
    boxes, mt, chunks = s.sph_bvh_refit(S, widen=False)
    assert boxes.tobytes() == d["boxes"].tobytes()
    assert np.isfinite(mt).all() and (mt > 0).all() and chunks.shape == ((n + 63) // 64, 4)
    wide, _, chunks2 = s.sph_bvh_refit(S.copy(), widen=True)
    assert (wide[:, :, :3] < boxes[:, :, :3]).all() and (wide[:, :, 3:] > boxes[:, :, 3:]).all()
    assert chunks.tobytes() == chunks2.tobytes()
    # the leaves hold every sphere once, in device order
    ids = d["leaf_ids"].reshape(-1)
    assert sorted(ids[ids >= 0].tolist()) == list(range(n)) and (ids[n:] == -1).all()
    assert np.array_equal(d["device_index"][ids[:n]], np.arange(n))


@pytest.mark.parametrize("key", list(SCENES))
def test_records_are_the_description_s(key):
    desc, s, _ = built(key)
    S = sph_data(desc)
    got = s.sph_records()
    assert got.shape == (len(S), _lib.RFX_SPH_RECORD_WORDS) and got.tobytes() == record_words(S).tobytes()


@pytest.mark.parametrize("key", list(SCENES))
def test_set_spheres_equals_a_fresh_build(key):
    desc = SCENES[key]()
    s, _ = build_scene(desc)
    S = sph_data(desc)
    before = s.sph_records()
    J = jiggle(S)
    v0 = s._version
    s.setSpheres(0, J)
    assert s._version > v0
    fresh, _ = build_scene(moved_desc(desc, J))
    a = s.sph_records()
    assert a.tobytes() == fresh.sph_records().tobytes() == record_words(J).tobytes()
    assert (a != before).any(axis=1).all()
    da, db = s.sph_bvh_dump(), fresh.sph_bvh_dump()
    for k in ("boxes", "children", "leaf_ids", "device_index"):
        assert np.array_equal(da[k], db[k]), k
    # a range in the middle leaves the others alone
    s2, _ = build_scene(desc)
    s2.setSpheres(10, J[10:21])
    c = s2.sph_records()
    assert c[10:21].tobytes() == a[10:21].tobytes()
    assert c[:10].tobytes() == before[:10].tobytes() and c[21:].tobytes() == before[21:].tobytes()


def test_set_spheres_clamps_as_the_constructor():
    eye = scenes.stress_scene(100).camera[0]
    Sp = special_spheres(eye)
    base = scenes.stress_scene(100)
    s, _ = build_scene(base)
    s.setSpheres(40, Sp)
    fresh, _ = build_scene(moved_desc(base, Sp, first=40))
    a = s.sph_records()
    assert a.tobytes() == fresh.sph_records().tobytes()
    assert a[40:40 + len(Sp)].tobytes() == record_words(Sp).tobytes()
    tiny = (np.float32(1.0842021724855044e-19) ** 2).astype(F).view(np.uint32)
    assert (a[40:43, 3] == tiny).all() and a[43, 3] == 0x7FC00000 and a[44, 3] == F(np.inf).view(np.uint32)


def test_scene_entry_errors():
    s, _ = build_scene(scenes.soup_scene(31, n_spheres=2))
    L = _lib.load()
    v = np.zeros(8, F)
    assert L.rfx_scene_set_spheres(s._h, 2, 1, _lib.fptr(v)) == -1
    assert L.rfx_scene_set_spheres(s._h, 0, 0, _lib.fptr(v)) == -1
    assert L.rfx_scene_set_spheres(s._h, 0, 1, None) == -1
    assert L.rfx_scene_set_spheres(None, 0, 1, _lib.fptr(v)) == -1
    assert L.rfx_scene_set_spheres(s._h, 0, 2, _lib.fptr(v)) == 0
    assert L.rfx_scene_object_sphere(s._h, 2) == -1 and L.rfx_scene_object_sphere(s._h, 99) == -1
    assert [s.object_sphere(k) for k in (0, 1)] == [0, 1]
    assert L.rfx_scene_sph_records(s._h, 1, 2, None) == -1
    d = s.sph_bvh_dump()  # at most 32 spheres: no pair tree, the device order is the insertion order
    assert d["nodes"] == 0 and d["device_index"].tolist() == [0, 1]


# ------------------------------------------------------------------------------------------------ containment
def contained(s, d, S):
    """every sphere's own box inside every child box on its path (widen = 0) and inside its chunk's bound"""
    boxes, _, chunks = s.sph_bvh_refit(S, widen=False)
    lo, hi = sphere_boxes(S)
    paths = tree_paths(d)
    assert sorted(paths) == list(range(len(S)))
    for i, p in paths.items():
        for (n, c) in p:
            b = boxes[n, c].astype(np.float64)
            assert (b[:3] <= lo[i]).all() and (b[3:] >= hi[i]).all(), (i, n, c)
    c = clamped(S).astype(np.float64)
    dev = d["device_index"]
    cb = chunks.astype(np.float64)[dev // 64]
    reach = np.linalg.norm(c[:, :3] - cb[:, :3], axis=1) + (clamped(S)[:, 3] * F(1.00001)).astype(np.float64)
    assert (reach <= cb[:, 3]).all(), int((reach > cb[:, 3]).sum())
    return boxes, chunks


@pytest.mark.parametrize("key", list(SCENES))
def test_containment_after_a_jiggle_and_a_shuffle_and_back(key):
    desc, s, d = built(key)
    A = sph_data(desc)
    box_a, chunk_a = contained(s, d, A)
    B, Cs = jiggle(A), shuffle(jiggle(A, seed=5))
    box_b, _ = contained(s, d, B)
    box_c, chunk_c = contained(s, d, Cs)
    assert box_b.tobytes() != box_a.tobytes() and box_c.tobytes() != box_b.tobytes()
    assert chunk_c.tobytes() != chunk_a.tobytes()
    # A -> B -> C -> A: a refit is a function of the spheres alone
    again, _, chunk_again = s.sph_bvh_refit(A.copy(), widen=False)
    assert again.tobytes() == box_a.tobytes() and chunk_again.tobytes() == chunk_a.tobytes()
    for widen in (False, True):
        assert s.sph_bvh_refit(A, widen)[0].tobytes() == s.sph_bvh_refit(A.copy(), widen)[0].tobytes()


# ------------------------------------------------------------------------------------------------ replay of the cull
def reported(o, d, S, i):
    """the reference's verdict for ray k on sphere i[k] of S (clamped radii, as the scene holds them)"""
    import oracle as orc
    c = clamped(S)
    rec = np.zeros((len(o), 11), F)
    rec[:, 0:3], rec[:, 3:6] = o, d
    rec[:, 6:10] = c[i]
    res = orc.kat("sphere", rec)
    return (res[:, 0] != 0) | (res[:, 14] != 0)


def path_boxes_kept(boxes, paths, i, o, d, ref, rng):
    """kept_prewide on every child box of the paths of spheres i for the rays (o, d): the number checked"""
    depth = max(len(paths[int(x)]) for x in i)
    checked = 0
    for lev in range(depth):
        sel = np.array([len(paths[int(x)]) > lev for x in i])
        nc = np.array([paths[int(x)][lev] for x in i[sel]])
        b = boxes[nc[:, 0], nc[:, 1]]
        k, _, _ = kept_prewide(b[:, :3], b[:, 3:], o[sel], d[sel], ref[None, :], rng)
        assert k.all(), (lev, int((~k).sum()), i[sel][~k][:8].tolist())
        checked += len(k)
    return checked


@pytest.mark.parametrize("move", ["jiggle", "shuffle"])
def test_refitted_boxes_keep_every_reported_hit(move):
    """2^16 rays from at least 20 units outside the scene box, each aimed at a point within 0.9 r of a moved sphere's
    centre: wherever the reference reports the sphere hit, the kernel's float32 box test keeps every widened child box
    on the sphere's path"""
    desc, s, d = built("soup1500s300")
    A = sph_data(desc)
    S = jiggle(A) if move == "jiggle" else shuffle(jiggle(A, seed=5))
    boxes, _, _ = s.sph_bvh_refit(S, widen=True)
    paths = tree_paths(d)
    ref = ref_point(A)
    rng = np.random.default_rng(SEED)
    n = 1 << 16
    i = rng.integers(0, len(S), n)
    c, r = S[i, :3].astype(np.float64), S[i, 3].astype(np.float64)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    target = c + u * (r * 0.9 * rng.random(n) ** (1 / 3))[:, None]
    lo, hi = sphere_boxes(S)
    lo, hi = lo.min(0), hi.max(0)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    o = 0.5 * (lo + hi) + v * (0.5 * np.linalg.norm(hi - lo) + np.exp(rng.uniform(np.log(20.0), np.log(2e4), n)))[:, None]
    assert (np.linalg.norm(np.maximum(np.maximum(lo - o, o - hi), 0.0), axis=1) >= 20.0).all()
    ray = (target - o) * np.exp(rng.uniform(np.log(0.1), np.log(10.0), n))[:, None]
    o32, d32 = o.astype(F), ray.astype(F)
    hit = reported(o32, d32, S, i)
    assert hit.sum() >= n // 2, int(hit.sum())
    checked = path_boxes_kept(boxes, paths, i[hit], o32[hit], d32[hit], ref, rng)
    assert checked > hit.sum() * 3


def special_scene():
    """stress100 with special_spheres over spheres 40 .. 51, built as it stands and moved: (Scene, dump, S, built S)"""
    desc = SCENES["stress100"]()
    _, s, d = built("stress100")
    A = sph_data(desc)
    S = jiggle(A)
    Sp = special_spheres(desc.camera[0])
    S[40:40 + len(Sp)] = Sp
    return s, d, S, A


def slab_overflows(o, d, ref):
    """rays for which a slab constant (o +- dm) rcp(d) of rfx_bvh.h ray_inv is not finite: the reciprocal is clamped to
    +-1e30 (a zero, tiny or NaN component), so an origin beyond 3.4e8 on that axis overflows it, and bvh_box then loses
    every box, finite or not, built or refitted (DESIGN.md "Moving meshes": "finite boxes are culled for such rays too")"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        o64, d64 = o.astype(np.float64), d.astype(np.float64)
        inv = np.nan_to_num(np.clip(1.0 / d64, -1e30, 1e30), nan=1e30)
        dm = 2.1e-3 * np.sqrt(((o64 - ref.astype(np.float64)) ** 2).sum(1)) + 1e-6
        return ~(((np.abs(o64) + dm[:, None]) * np.abs(inv)).max(axis=1) < 3.0e38)


def test_edge_rays_on_the_special_spheres():
    """zero, axis-parallel, infinite and NaN directions from origins out to 1e30 against the refitted boxes of a scene
    holding the special spheres: a sphere the reference reports hit has every box on its path kept.  Left out, by name:
    the rays of slab_overflows, which lose the boxes of a fresh build as well."""
    s, d, S, A = special_scene()
    boxes, _, _ = s.sph_bvh_refit(S, widen=True)
    paths = tree_paths(d)
    ref = ref_point(A)
    rng = np.random.default_rng(7)
    vals = np.array([0.0, -0.0, 1.0, -1.0, 1e-30, -1e-38, 1e30, -1e30, 3e38, np.inf, -np.inf, np.nan], F)
    D = np.stack(np.meshgrid(vals, vals, vals, indexing="ij"), -1).reshape(-1, 3)
    origins = np.array([0.0, -0.0, 1.0, -7.5, 1e-20, 1e10, -1e20, 1e30, -1e30], F)
    O = np.stack(np.meshgrid(origins, origins, origins, indexing="ij"), -1).reshape(-1, 3)
    spheres = np.concatenate([np.arange(40, 52), rng.integers(0, len(S), 12)])
    nr = len(D) * 4
    d32 = np.tile(D, (4, 1))
    o32 = O[rng.integers(0, len(O), nr)]
    # half of the origins near the sphere instead, so that the axis-parallel rays meet it
    near = rng.random(nr) < 0.5
    total, seen = 0, set()
    for sph in spheres:
        reach = 4.0 * max(1.0, float(np.nan_to_num(np.abs(S[sph]).max(), nan=1.0, posinf=1.0)))
        with np.errstate(invalid="ignore", over="ignore"):
            o = np.where(near[:, None], (S[sph, :3] + rng.uniform(-reach, reach, (nr, 3))).astype(F), o32)
        # ... and a quarter of the rays along an axis straight at it, from 1 to 1e12 radii away
        dd = d32.copy()
        c4 = clamped(S)[sph].astype(np.float64)
        if np.isfinite(c4).all():
            m = nr // 4
            ax, sign = rng.integers(0, 3, m), rng.choice([-1.0, 1.0], m)
            off = rng.uniform(-0.6, 0.6, (m, 3)) * c4[3]
            off[np.arange(m), ax] = sign * c4[3] * 10.0 ** rng.uniform(0.0, 12.0, m)
            aim = np.zeros((m, 3))
            aim[np.arange(m), ax] = -sign
            with np.errstate(over="ignore"):
                o[:m], dd[:m] = (c4[:3] + off).astype(F), aim.astype(F)
            # ... and another quarter from a random side, 2 to 1e3 radii away, at a point inside it
            u = rng.normal(size=(m, 3))
            u /= np.linalg.norm(u, axis=1)[:, None]
            start = c4[:3] + u * (c4[3] * 10.0 ** rng.uniform(0.3, 3.0, m))[:, None]
            o[m:2 * m] = start.astype(F)
            aim = c4[:3] + rng.uniform(-0.5, 0.5, (m, 3)) * c4[3] - start
            with np.errstate(invalid="ignore"):  # (unit: a 1e15 ray squared overflows; 0 / 0 at the 1e-19 radius)
                dd[m:2 * m] = (aim / np.linalg.norm(aim, axis=1)[:, None]).astype(F)
        i = np.full(nr, sph)
        hit = reported(o, dd, S, i) & ~slab_overflows(o, dd, ref)
        if hit.any():
            total += path_boxes_kept(boxes, paths, i[hit], o[hit], dd[hit], ref, rng)
            seen.add(int(sph))
    # (not empty: the finite specials and the ordinary spheres are all met)
    assert seen >= {40, 41, 42, 48, 49, 50, 51} | set(int(x) for x in spheres[12:]), sorted(seen)
    # the spheres that are not finite report nothing, from anywhere (the one at 1e30 is met from origins out there)
    for k in (3, INFINITE_RADIUS, 5, INFINITE_CENTRE):
        i = np.full(nr, 40 + k)
        assert not reported(o32, d32, S, i).any()
    # the infinite radius: every child above it is all of space (NaN bounds), as above an ill-conditioned triangle
    for (n, c) in paths[40 + INFINITE_RADIUS]:
        assert (boxes[n, c].view(np.uint32) == 0x7FC00000).all()


def test_an_infinite_centre_makes_infinite_boxes():
    """A centre component of +inf: the leaf's box is infinite on that axis, the builder's widening is infinite, and all six
    bounds of every child above the sphere come out infinite with a NaN margin term.  The sphere itself is never
    reported hit, and an infinite box is kept by every ray whose slab constants are finite.  The known limit (DESIGN.md
    "Moving spheres -> Spheres that are not finite"): a ray with a zero direction component from beyond 3.4e8 on that
    axis overflows its slab constant and loses the box, so a sphere that far out under the same boxes can be missed
    after the update, where a fresh build -- whose reference point is then not finite either -- keeps it."""
    s, d, S, A = special_scene()
    S[40 + INFINITE_RADIUS] = jiggle(A)[40 + INFINITE_RADIUS]
    boxes, mt, chunks = s.sph_bvh_refit(S, widen=True)
    paths = tree_paths(d)
    sph = 40 + INFINITE_CENTRE
    for (n, c) in paths[sph]:
        assert np.isinf(boxes[n, c]).all() and (boxes[n, c, :3] < 0).all() and (boxes[n, c, 3:] > 0).all()
        assert mt[n, c].view(np.uint32) == 0x7FC00000
    rng = np.random.default_rng(3)
    o = rng.uniform(-30, 30, (4096, 3)).astype(F)
    ray = rng.normal(size=(4096, 3)).astype(F)
    assert not reported(o, ray, S, np.full(4096, sph)).any()
    ref = ref_point(A)
    b = boxes[paths[sph][-1]][None].repeat(4096, 0)
    kept, t0, t1 = kept_prewide(b[:, :3], b[:, 3:], o, ray, ref[None, :], rng)
    assert kept.all() and (t0 == 0).all() and np.isinf(t1).all()
    # its chunk's bound is not finite: cull_chunk's !(L > rp && va < lim) keeps it
    assert not np.isfinite(chunks[d["device_index"][sph] // 64, 3])
    # the limit: straight up the y axis at the sphere 1e15 away, from x = 1e15
    far = 48
    o1 = (S[far, :3].astype(np.float64) + (0.0, -1e15, 0.0)).astype(F)[None]
    d1 = np.array([[0.0, 1.0, 0.0]], F)
    assert reported(o1, d1, S, np.array([far])).all()
    shared = [nc for nc in paths[far] if nc in paths[sph]]
    assert shared
    b1 = boxes[shared[-1]][None]
    assert not kept_prewide(b1[:, :3], b1[:, 3:], o1, d1, ref[None, :], rng)[0][0]
