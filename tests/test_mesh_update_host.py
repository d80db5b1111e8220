"""Moving meshes, the host side (rfx.h "Moving meshes"; no device): rfx_scene_set_triangle_vertices against a scene
built at the same vertices, the host refit against the builder's own boxes, and the soundness of the refitted boxes --
the device copy and the all-space (NaN) box of a triangle that turned ill-conditioned -- on the float32 replay of the
kernel's box test, against the reference's verdicts (oracle.kat("triangle"))."""
import os
import re

import numpy as np
import pytest

from mesh_update import F, case1_vertices, kept_prewide, moved_desc, tree_paths, tri_vertices, wave
from reflaxman_amd import _lib, scenes
from reflaxman_amd.render import build_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def refit_scenes():
    return {"mesh16x12": scenes.mesh_scene(16, 12), "soup300_degenerate": scenes.degenerate_soup_scene(),
            "soup33": scenes.soup_scene(31)}


def test_cond_threshold_is_the_root_s_preimage_of_300():
    """rfx_refit.h kTriCondSq: p < kTriCondSq <=> sqrt(p) < 300 (the root is monotone, so its two neighbours decide)"""
    text = open(os.path.join(ROOT, "reflaxman_amd", "csrc", "rfx_refit.h")).read()
    t = float.fromhex(re.search(r"kTriCondSq = (0x[0-9a-fp.+-]+);", text).group(1))
    assert np.sqrt(np.float64(t)) >= 300.0 and np.sqrt(np.nextafter(np.float64(t), 0.0)) < 300.0


def test_set_triangle_vertices_equals_a_fresh_build():
    """300 triangles (soup, slivers, zero-area, coincident, 1e30-sized, subnormal-sized, NaN and infinite vertices)
    set in place on a scene built elsewhere: every word that follows a vertex is the fresh scene's, as bits"""
    V = case1_vertices()
    base = scenes.soup_scene(298, n_spheres=8)
    assert base.n_triangles == 300
    s, _ = build_scene(base)
    before = s.tri_records()
    v0 = s._version
    s.setTriangleVertices(0, V)
    assert s._version > v0
    fresh, _ = build_scene(moved_desc(base, V))
    a, b = s.tri_records(), fresh.tri_records()
    assert a.shape == (300, _lib.RFX_TRI_RECORD_WORDS) and a.tobytes() == b.tobytes()
    assert (a != before).any(axis=1).sum() > 290
    assert 200 < a[:, 28].sum() <= 300 - 14 - 8 and (a[-8:, 28] == 0).all()  # slivers, zero areas and the specials
    assert (a[a[:, 28] == 0, 18] == np.float32(np.inf).view(np.uint32)).all()  # never culled
    # the vertices are kept as given (NaNs canonical), and a range in the middle leaves the others alone
    given = V.reshape(300, 9).view(np.uint32).copy()
    given[np.isnan(V.reshape(300, 9))] = 0x7FC00000
    assert np.array_equal(a[:, 19:28], given)
    s2, _ = build_scene(base)
    s2.setTriangleVertices(100, V[100:117])
    c = s2.tri_records()
    assert c[100:117].tobytes() == a[100:117].tobytes()
    assert c[:100].tobytes() == before[:100].tobytes() and c[117:].tobytes() == before[117:].tobytes()
    # the tree and the residual list of the edited scene are the fresh scene's
    da, db = s.tri_bvh_dump(), fresh.tri_bvh_dump()
    for k in ("boxes", "children", "leaf_ids", "residual"):
        assert np.array_equal(da[k], db[k]), k


def test_scene_entry_errors():
    s, _ = build_scene(scenes.soup_scene(31, n_spheres=2))
    L = _lib.load()
    v = np.zeros(9, F)
    assert L.rfx_scene_set_triangle_vertices(s._h, 33, 1, _lib.fptr(v)) == -1
    assert L.rfx_scene_set_triangle_vertices(s._h, 0, 0, _lib.fptr(v)) == -1
    assert L.rfx_scene_set_triangle_vertices(s._h, 0, 1, None) == -1
    assert L.rfx_scene_set_triangle_vertices(s._h, 32, 1, _lib.fptr(v)) == 0
    assert L.rfx_scene_object_triangle(s._h, 0) == -1 and L.rfx_scene_object_triangle(s._h, 99) == -1
    assert [s.object_triangle(k) for k in (2, 3, 34)] == [0, 1, 32]  # two spheres first
    assert L.rfx_scene_tri_records(s._h, 30, 4, None) == -1


@pytest.mark.parametrize("name", ["mesh16x12", "soup300_degenerate", "soup33"])
def test_refit_to_the_scene_s_own_vertices_is_the_dump(name):
    desc = refit_scenes()[name]
    s, _ = build_scene(desc)
    d = s.tri_bvh_dump()
    if name == "soup33":
        assert d["leaves"] == 9 and (d["leaf_ids"][8] >= 0).sum() == 1
    boxes, mt = s.tri_bvh_refit(tri_vertices(desc), widen=False)
    assert boxes.tobytes() == d["boxes"].tobytes()
    assert np.isfinite(mt).all() and (mt > 0).all()
    # the device copy holds the boxes as built, and a refit is a function of the vertices alone
    wide, _ = s.tri_bvh_refit(tri_vertices(desc), widen=True)
    assert (wide[:, :, :3] < boxes[:, :, :3]).all() and (wide[:, :, 3:] > boxes[:, :, 3:]).all()
    V = wave(tri_vertices(desc))
    assert s.tri_bvh_refit(V, widen=True)[0].tobytes() == s.tri_bvh_refit(V.copy(), widen=True)[0].tobytes()
    assert s.tri_bvh_refit(tri_vertices(desc), widen=True)[0].tobytes() == wide.tobytes()


def moved_degenerate():
    """soup300_degenerate with every triangle on a wave and six in-tree triangles turned into slivers, a zero-area
    triangle and a NaN vertex: (built Scene, dump, moved vertices, the six)"""
    desc = scenes.degenerate_soup_scene()
    s, _ = build_scene(desc)
    d = s.tri_bvh_dump()
    V = wave(tri_vertices(desc), amp=0.4)
    six = [int(t) for t in d["leaf_ids"][[0, 3, 17, 30, 41, 55], 0]]
    for k, t in enumerate(six[:4]):  # slivers: the third vertex 1e-4 of the first edge off its line
        a, b = V[t, 0].astype(np.float64), V[t, 1].astype(np.float64)
        V[t, 2] = (a + 0.3 * (b - a) + 1e-4 * np.linalg.norm(b - a) * np.roll(np.eye(3)[k % 3], 1)).astype(F)
    V[six[4], 2] = V[six[4], 1]
    V[six[5], 0, 1] = np.nan
    return s, d, V, six


def test_refitted_boxes_keep_every_reported_hit():
    """rays aimed near the edges and vertices of the moved triangles: every box on the root-to-leaf path of a triangle
    the reference reports as hit is kept by the kernel's float32 box test, the all-space boxes above the six included"""
    import oracle as orc
    s, d, V, six = moved_degenerate()
    boxes, mt = s.tri_bvh_refit(V, widen=True)
    paths = tree_paths(d)
    # the six's leaves and every child above them are all of space; the others are finite
    ill = np.zeros(boxes.shape[:2], bool)
    for t in six:
        for (n, c) in paths[t]:
            ill[n, c] = True
    assert (boxes[ill].view(np.uint32) == 0x7FC00000).all() and np.isinf(mt[ill]).all()
    assert np.isfinite(boxes[~ill]).all() and np.isfinite(mt[~ill]).all()
    tree = np.array(sorted(paths), np.int64)
    V0 = tri_vertices(scenes.degenerate_soup_scene())
    well = np.ones(len(V0), bool)
    well[d["residual"]] = False
    pts = V0[well].reshape(-1, 3).astype(np.float64)
    ref = (0.5 * (pts.min(0) + pts.max(0))).astype(F)  # rfx_scene.cpp tri_ref_point
    rng = np.random.default_rng(1350490027)
    n = 1 << 16
    t = tree[rng.integers(0, len(tree), n)]
    t[::16] = np.array(six)[rng.integers(0, 5, len(t[::16]))]  # (not the NaN one: it reports nothing)
    W = V[t].astype(np.float64)
    k = rng.integers(0, 3, n)
    A, B = W[np.arange(n), k], W[np.arange(n), (k + 1) % 3]
    sp = np.where(rng.random(n) < 0.3, 0.0, rng.random(n))
    p = A + (B - A) * sp[:, None]
    nrm = np.cross(W[:, 1] - W[:, 0], W[:, 2] - W[:, 0])
    ln = np.linalg.norm(nrm, axis=1)
    nrm = np.where(ln[:, None] > 0, nrm / np.where(ln > 0, ln, 1.0)[:, None], (0.0, 1.0, 0.0))
    out = np.cross(B - A, nrm)
    lo_ = np.linalg.norm(out, axis=1)
    out = np.where(lo_[:, None] > 0, out / np.where(lo_ > 0, lo_, 1.0)[:, None], (1.0, 0.0, 0.0))
    size = np.maximum(np.linalg.norm(W[:, 1] - W[:, 0], axis=1), 1e-3)
    dist = size * np.exp(rng.uniform(np.log(0.05), np.log(2000.0), n))
    eps = rng.normal(0.0, 1.0, n) * np.exp(rng.uniform(np.log(1e-7), np.log(1e-2), n))
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    o = p + u * dist[:, None]
    ray = (p + out * (eps * dist)[:, None] - o) * np.exp(rng.uniform(np.log(0.1), np.log(10.0), n))[:, None]
    rec = np.zeros((n, 21), F)
    rec[:, 0:3], rec[:, 3:6] = o, ray
    rec[:, 6:15] = V[t].reshape(n, 9)
    res = orc.kat("triangle", rec)
    hit = (res[:, 0] != 0) | (res[:, 14] != 0)
    assert hit.sum() > n // 8 and hit[::16].sum() > 16
    o32, d32 = rec[hit, 0:3], rec[hit, 3:6]
    th = t[hit]
    depth = max(len(paths[int(x)]) for x in th)
    checked = 0
    for lev in range(depth):
        sel = np.array([len(paths[int(x)]) > lev for x in th])
        nc = np.array([paths[int(x)][lev] for x in th[sel]])
        b = boxes[nc[:, 0], nc[:, 1]]
        k_, _, _ = kept_prewide(b[:, :3], b[:, 3:], o32[sel], d32[sel], ref[None, :], rng)
        assert k_.all(), (lev, int((~k_).sum()))
        checked += len(k_)
    assert checked > hit.sum() * 3


def test_all_space_box_is_kept_by_every_ray():
    """the all-space child (NaN bounds): t0 = 0 and the cull's comparison fails for axis-parallel, zero, infinite and NaN
    directions and origins up to 1e30.  Infinite bounds are not all of space to this test: where (o + dm) rcp(d)
    overflows, inf - inf leaves one slab end NaN and the other, -inf, is taken for both"""
    rng = np.random.default_rng(7)
    vals = np.array([0.0, -0.0, 1.0, -1.0, 1e-30, -1e-38, 1e30, -1e30, 3e38, np.inf, -np.inf, np.nan], F)
    d = np.stack(np.meshgrid(vals, vals, vals, indexing="ij"), -1).reshape(-1, 3)
    origins = np.array([0.0, -0.0, 1.0, -7.5, 1e-20, 1e10, -1e20, 1e30, -1e30], F)
    o = np.stack(np.meshgrid(origins, origins, origins, indexing="ij"), -1).reshape(-1, 3)
    oi = rng.integers(0, len(o), len(d) * 8)
    D, O = np.tile(d, (8, 1)), o[oi]
    q = np.full_like(D, np.nan)
    for ref in (np.zeros(3, F), np.array([3.0, -2.0, 1e3], F)):
        k, t0, t1 = kept_prewide(q, q, O, D, ref[None, :], rng)
        assert k.all() and (t0 == 0).all() and np.isnan(t1).all()
    # the reason the bounds are not +-inf: an axis-parallel ray from 1e10 is lost
    O1, D1 = np.array([[1e10, 0.0, 0.0]], F), np.array([[0.0, 1.0, 0.0]], F)
    k, _, t1 = kept_prewide(np.full_like(D1, -np.inf), np.full_like(D1, np.inf), O1, D1, np.zeros((1, 3), F), rng)
    assert not k[0] and t1[0] == -np.inf
