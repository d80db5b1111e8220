"""Re-cutting, the host side (rfx.h "Re-cutting"; no device): rfx_scene_tri_bvh_recut against a numpy float32
restatement of the cut (tests/recut_helpers.py), its leaf and box edge cases, the refit's boxes on the new topology, and
the soundness of those boxes on the float32 replay of the kernel's box test against the reference's verdicts."""
import numpy as np
import pytest

import recut_helpers as rh
from mesh_update import F, kept_prewide, special_triangles, tree_paths, tri_vertices, wave
from reflaxman_amd import _lib, scenes
from reflaxman_amd.render import build_scene

_CASE = {}
SCENES = {"mesh16x12": lambda: scenes.mesh_scene(16, 12), "soup33": lambda: scenes.soup_scene(31),
          "soup302": lambda: scenes.soup_scene(300), "degenerate": scenes.degenerate_soup_scene,
          "soup4202": lambda: scenes.soup_scene(4200), "soup63": lambda: scenes.soup_scene(61),
          "soup64": lambda: scenes.soup_scene(62)}


def case(name):
    """(description, built Scene, its dump, its vertices, the in-tree list), built once and never edited"""
    if name not in _CASE:
        desc = SCENES[name]()
        s, _ = build_scene(desc)
        d = s.tri_bvh_dump()
        V = tri_vertices(desc)
        _CASE[name] = (desc, s, d, V, rh.in_tree(d, len(V)))
    return _CASE[name]


def cut_vertices(V, how):
    return {"own": lambda: V, "wave": lambda: wave(V, amp=0.4), "shuffle": lambda: rh.shuffle(V)}[how]()


def check_membership(r, d, tree):
    ids = r["leaf_ids"]
    got = ids[ids >= 0]
    assert np.array_equal(np.sort(got), tree) and len(np.unique(got)) == len(got)  # each in-tree triangle exactly once
    assert not np.isin(d["residual"], got).any()
    assert (ids.reshape(-1)[:len(tree)] >= 0).all() and (ids.reshape(-1)[len(tree):] == -1).all()  # padding last
    assert (r["nodes"], r["leaves"]) == (d["nodes"], d["leaves"]) == (d["leaves"] - 1, -(-len(tree) // rh.LEAF))
    assert r["depth"] == (r["leaves"] - 1).bit_length()  # ceil(log2 G)
    assert np.array_equal(r["residual"], d["residual"])


@pytest.mark.parametrize("how", ["own", "wave", "shuffle"])
@pytest.mark.parametrize("name", ["mesh16x12", "soup33", "soup302", "degenerate", "soup4202"])
def test_cut_equals_the_restatement(name, how):
    desc, s, d, V, tree = case(name)
    C = cut_vertices(V, how)
    r = s.tri_bvh_recut(C)
    want = rh.restated(C, rh.classes(desc, C), tree)
    assert np.array_equal(r["leaf_ids"], want["leaf_ids"])
    assert np.array_equal(r["children"], want["children"])
    assert r["depth"] == want["depth"]
    check_membership(r, d, tree)
    if name == "degenerate" and how == "own":
        assert len(d["residual"]) == 14
        k = want["keys"]
        assert (np.bincount(k[want["placed"]] & 0x3FFFFFFF).max() >= 2) and want["placed"].all()  # coincident pairs
    if name == "soup4202":
        assert len(tree) > _lib.RFX_ORDER_TILE
    if how == "shuffle":  # (a low wave over a flat mesh need not move a triangle to another cubic cell)
        assert not np.array_equal(r["leaf_ids"], s.tri_bvh_recut(V)["leaf_ids"])


def test_leaf_edges():
    """in-tree counts with T mod 4 in {0, 1, 3}, a power-of-two leaf count and others"""
    seen = set()
    for name in ("soup64", "soup33", "soup63", "degenerate"):
        desc, s, d, V, tree = case(name)
        r = s.tri_bvh_recut(rh.shuffle(V))
        check_membership(r, d, tree)
        G = r["leaves"]
        seen.add((len(tree) % 4, G & (G - 1) == 0))
        assert (r["leaf_ids"][-1] >= 0).sum() == (len(tree) - 1) % 4 + 1
        kids, depth = rh.cut_topology(G)
        assert np.array_equal(r["children"], kids) and r["depth"] == depth
    assert {(0, True), (1, False), (3, True), (2, False)} <= seen


def test_degenerate_boxes():
    desc, s, d, V, tree = case("mesh16x12")
    # every centroid equal: scale 0, every key 0, index order
    same = np.broadcast_to(V[5], V.shape).copy()
    r = s.tri_bvh_recut(same)
    assert np.array_equal(r["leaf_ids"].reshape(-1)[:len(tree)], tree)
    assert rh.cut_keys(same[tree], np.zeros(len(tree)))[4] == 0
    # a planar mesh: one axis of zero extent
    flat = V.copy()
    flat[..., 1] = 0.0
    want = rh.restated(flat, rh.classes(desc, flat), tree)
    assert want["lo"][1] == want["hi"][1] == 0 and want["scale"] > 0 and want["placed"].all()
    r = s.tri_bvh_recut(flat)
    assert np.array_equal(r["leaf_ids"], want["leaf_ids"])
    assert (want["keys"] & 0x12492492).sum() == 0 and len(np.unique(want["keys"])) > 32  # no y bit is ever set
    # a bound of -0.0 against +0.0: the same keys, whichever zero the minimum kept
    for pick in (slice(0, None, 2), slice(1, None, 2), slice(0, 1), slice(None)):
        signed = flat.copy()
        signed[pick, :, 1] = -0.0
        assert np.signbit(signed[..., 1]).any()
        assert np.array_equal(s.tri_bvh_recut(signed)["leaf_ids"], r["leaf_ids"])
    # ... and on an axis that has an extent: the lowest sum at -0.0 or at +0.0
    step = flat.copy()
    step[::3, :, 1] = 4.0  # every third triangle lifted whole: lo_y = +-0, hi_y = 12
    base = rh.restated(step, rh.classes(desc, step), tree)
    assert base["lo"][1] == 0 and base["hi"][1] == 12 and (base["keys"] & 0x12492492).any()
    assert np.array_equal(s.tri_bvh_recut(step)["leaf_ids"], base["leaf_ids"])
    for pick in (slice(1, None, 3), slice(2, None, 3), slice(1, 2)):
        signed = step.copy()
        signed[pick, :, 1] = -0.0
        assert np.array_equal(s.tri_bvh_recut(signed)["leaf_ids"], base["leaf_ids"])


def ill_case():
    """soup302 with make_ill's six and special_triangles() written over in-tree triangles of a shuffle"""
    desc, s, d, V, tree = case("soup302")
    six = [int(t) for t in d["leaf_ids"][[0, 3, 17, 30, 41, 55], 0]]
    spec = [int(t) for t in d["leaf_ids"][[5, 9, 22, 33, 47, 60, 66, 70], 1]]
    C = rh.make_ill(rh.shuffle(V), six)
    C[spec] = special_triangles()
    return desc, s, d, C, tree, six + spec


def test_ill_triangles_take_the_last_leaves():
    desc, s, d, C, tree, bad = ill_case()
    ill = rh.classes(desc, C)
    assert ill[bad].all() and ill.sum() == len(bad)
    r = s.tri_bvh_recut(C, widen=True)
    want = rh.restated(C, ill, tree)
    assert np.array_equal(r["leaf_ids"], want["leaf_ids"])
    assert (want["keys"][np.isin(tree, bad)] == rh.LAST_KEY).all() and (want["keys"][~np.isin(tree, bad)] < rh.LAST_KEY).all()
    flat = r["leaf_ids"].reshape(-1)
    assert np.array_equal(flat[len(tree) - len(bad):len(tree)], np.sort(bad))  # last, in ascending index
    # the placed triangles' box ignores them: other ill vertices in their place, the same order
    other = C.copy()
    other[bad] = F(1e20)
    assert np.array_equal(s.tri_bvh_recut(other)["leaf_ids"], r["leaf_ids"])
    # their leaves and every child above are all of space, and every other box holds the vertices beneath it
    paths = tree_paths(r)
    nan = np.zeros(r["boxes"].shape[:2], bool)
    for t in bad:
        for (n, c) in paths[t]:
            nan[n, c] = True
    assert (r["boxes"][nan].view(np.uint32) == rh.NAN_WORD).all() and np.isinf(r["mt"][nan]).all()
    assert np.isfinite(r["boxes"][~nan]).all() and np.isfinite(r["mt"][~nan]).all()
    assert nan.sum() < 3 * r["depth"]  # one spine, and the few leaves beside it
    for t in tree[~np.isin(tree, bad)]:
        for (n, c) in paths[int(t)]:
            if not nan[n, c]:
                assert (r["boxes"][n, c, :3] < C[t].min(0)).all() and (r["boxes"][n, c, 3:] > C[t].max(0)).all()


@pytest.mark.parametrize("widen", [False, True])
def test_boxes_fitted_to_other_vertices(widen):
    """cut at one vertex set, fitted to another: the builder's box formula on the re-cut topology, bit for bit"""
    for name in ("soup33", "degenerate"):
        desc, s, d, V, tree = case(name)
        C, W = rh.shuffle(V), wave(rh.shuffle(V, amp=2.0, seed=5), amp=0.7)
        if name == "degenerate":
            W = rh.make_ill(W, [int(tree[7])])
        r = s.tri_bvh_recut(C, W, widen=widen)
        cut = s.tri_bvh_recut(C, widen=widen)
        assert np.array_equal(r["leaf_ids"], cut["leaf_ids"]) and np.array_equal(r["children"], cut["children"])
        assert r["boxes"].tobytes() != cut["boxes"].tobytes()
        boxes, mt = rh.fitted(r["leaf_ids"], r["children"], W, rh.classes(desc, W), rh.ref_point(V, d["residual"]), widen)
        assert np.array_equal(rh.words(r["boxes"]), rh.words(boxes))
        assert np.array_equal(rh.words(r["mt"]), rh.words(mt))
        # vertices = None is the cut's own
        assert s.tri_bvh_recut(C, C, widen=widen)["boxes"].tobytes() == cut["boxes"].tobytes()


def test_recut_boxes_keep_every_reported_hit():
    """the moving-mesh host test's check on the new tree: soup300_degenerate shuffled, six in-tree triangles turned ill,
    re-cut; every box on the root-to-leaf path of a triangle the reference reports as hit is kept by the kernel's
    float32 box test"""
    import oracle as orc
    desc, s, d, V, tree = case("degenerate")
    six = [int(t) for t in d["leaf_ids"][[0, 3, 17, 30, 41, 55], 0]]
    C = rh.make_ill(rh.shuffle(V), six)
    r = s.tri_bvh_recut(C, widen=True)
    paths = tree_paths(r)
    ref = rh.ref_point(V, d["residual"])
    rec, t, rng = rh.edge_rays(C, tree, six[:5])  # (not the NaN one: it reports nothing)
    res = orc.kat("triangle", rec)
    hit = (res[:, 0] != 0) | (res[:, 14] != 0)
    n = len(rec)
    assert hit.sum() > n // 8 and hit[::16].sum() > 16
    o32, d32, th = rec[hit, 0:3], rec[hit, 3:6], t[hit]
    checked = 0
    for lev in range(r["depth"]):
        sel = np.array([len(paths[int(x)]) > lev for x in th])
        nc = np.array([paths[int(x)][lev] for x in th[sel]])
        b = r["boxes"][nc[:, 0], nc[:, 1]]
        k_, _, _ = kept_prewide(b[:, :3], b[:, 3:], o32[sel], d32[sel], ref[None, :], rng)
        assert k_.all(), (lev, int((~k_).sum()))
        checked += len(k_)
    assert checked > hit.sum() * 3


def test_entry_errors_and_scenes_without_a_tree():
    L = _lib.load()
    desc, s, d, V, tree = case("soup33")
    cnt = (_lib.C.c_int32 * 5)()
    v = np.ascontiguousarray(V.reshape(-1, 9))
    assert L.rfx_scene_tri_bvh_recut(None, _lib.fptr(v), None, 0, cnt, None, None, None, None) == -1
    assert L.rfx_scene_tri_bvh_recut(s._h, None, None, 0, cnt, None, None, None, None) == -1
    assert L.rfx_scene_tri_bvh_recut(s._h, _lib.fptr(v), None, 2, cnt, None, None, None, None) == -1
    assert L.rfx_scene_tri_bvh_recut(s._h, _lib.fptr(v), None, 0, cnt, None, None, None, None) == 1
    assert list(cnt) == [d["nodes"], d["leaves"], 0, rh.LEAF, (d["leaves"] - 1).bit_length()]
    small, _ = build_scene(scenes.default_scene())
    n = small.counts()[1]
    assert small.tri_bvh_recut(np.zeros((n, 3, 3), F)) is None
