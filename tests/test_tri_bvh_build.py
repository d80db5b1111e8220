"""The host builder of the triangle BVH, through rfx_scene_tri_bvh_dump (no renderer, no device).

Every triangle sits in exactly one leaf or in the residual list; ill-conditioned and singular triangles are
residual; each child box holds every vertex beneath it; depth and node count stay within what the kernels' int16
stack of kBvhStack = 16 slots can walk; rfx_scene_add_mesh builds the scene the per-triangle calls build.
"""
import ctypes as C

import numpy as np
import pytest

from reflaxman_amd import _lib, scenes
from reflaxman_amd.render import Color, Material, Scene, Vector3, build_scene

BVH_STACK, MAX_NODES = 16, 32767


def tri_vertices(desc):
    return np.array([[ob[1], ob[2], ob[3]] for ob in desc.objects if ob[0] == "triangle"], np.float32)


def basis_cond(v):
    """||M||_F ||M^-1||_F of the reference's basis [v2 - v0 | v1 - v0 | -norm] in double (inf: singular)."""
    v = v.astype(np.float64)
    a, b = v[2] - v[0], v[1] - v[0]
    n = np.cross(b, a)
    ln = np.linalg.norm(n)
    if ln == 0.0:
        return np.inf
    m = np.stack([a, b, -n / ln], axis=1)
    if abs(np.linalg.det(m)) < 1e-30:
        return np.inf
    return np.linalg.norm(m) * np.linalg.norm(np.linalg.inv(m))


def check_tree(desc, expect_tree=True):
    s, _ = build_scene(desc)
    d = s.tri_bvh_dump()
    V = tri_vertices(desc)
    if d is None:
        assert not expect_tree, desc.name
        return None
    assert d["depth"] <= BVH_STACK and 0 < d["nodes"] <= MAX_NODES and d["leaves"] <= MAX_NODES + 1, desc.name
    ids, res = d["leaf_ids"], d["residual"]
    assert ids.shape == (d["leaves"], d["leaf_size"])
    inside = ids[ids >= 0]
    assert (ids >= -1).all() and inside.max() < len(V)
    # exactly one home per triangle
    count = np.bincount(np.concatenate([inside, res]), minlength=len(V))
    assert (count == 1).all(), (desc.name, np.flatnonzero(count != 1)[:8].tolist())
    # ill-conditioned and singular triangles are residual (0.1% slack on the double restatement of the condition
    # number: the host computes it from the float basis and the float inverse)
    cond = np.array([basis_cond(v) for v in V])
    in_res = np.zeros(len(V), bool)
    in_res[res] = True
    assert in_res[cond >= 300.0 * 1.001].all(), desc.name
    assert not in_res[cond < 300.0 / 1.001].any(), desc.name
    # each child box holds every vertex beneath it; walk from the root with an explicit stack, measuring the depth
    kids, boxes = d["children"], d["boxes"]
    seen_nodes, seen_leaves = np.zeros(d["nodes"], bool), np.zeros(d["leaves"], bool)

    def under(c):
        """(lo, hi, internal levels) of subtree c, asserting its inner boxes on the way"""
        if c < 0:
            assert not seen_leaves[~c]
            seen_leaves[~c] = True
            t = ids[~c][ids[~c] >= 0]
            assert len(t) > 0
            p = V[t].reshape(-1, 3)
            return p.min(0), p.max(0), 0
        assert not seen_nodes[c]
        seen_nodes[c] = True
        lo, hi, lev = [], [], 0
        for k in range(2):
            l, h, dd = under(int(kids[c, k]))
            assert (boxes[c, k, :3] <= l).all() and (boxes[c, k, 3:] >= h).all(), (desc.name, c, k)
            lo.append(l); hi.append(h); lev = max(lev, dd)
        return np.minimum(*lo), np.maximum(*hi), lev + 1

    _, _, depth = under(0)
    assert seen_nodes.all() and seen_leaves.all()
    assert depth == d["depth"]
    return d


@pytest.mark.parametrize("n", [33, 65, 127, 129, 1500])
def test_soup_tree(n):
    d = check_tree(scenes.soup_scene(n))
    assert d["leaves"] == -(-(n + 2 - len(d["residual"])) // d["leaf_size"])  # the soup and the ground quad


def test_mesh_tree():
    d = check_tree(scenes.mesh_scene(16, 12))
    assert len(d["residual"]) == 0


def test_degenerate_tree():
    desc = scenes.degenerate_soup_scene()
    d = check_tree(desc)
    nt = desc.n_triangles
    # the 12 slivers and the 2 zero-area triangles precede the 8 coincident ones at the end of the scene
    assert set(range(nt - 22, nt - 8)) <= set(d["residual"].tolist())
    assert not set(range(nt - 8, nt)) & set(d["residual"].tolist())


def test_small_scene_has_no_tree():
    s, _ = build_scene(scenes.default_scene())
    assert s.tri_bvh_dump() is None


def test_large_mesh_meets_limits_or_reports_none():
    """132,000 triangles: more leaves than an int16 stack slot can name at 4 per leaf -- limits met, or no tree."""
    desc = scenes.mesh_scene(300, 220)
    assert desc.n_triangles == 132000
    V = tri_vertices(desc)
    idx = np.arange(3 * len(V), dtype=np.uint32).reshape(-1, 3)
    s = Scene(Color(1, 1, 1), 0.1)
    s.addMesh(V.reshape(-1, 3), idx, Material())
    cnt = (C.c_int32 * 5)()
    rc = _lib.check(_lib.load().rfx_scene_tri_bvh_dump(s._h, cnt, None, None, None, None))
    if rc:
        assert cnt[4] <= BVH_STACK and cnt[0] <= MAX_NODES and cnt[1] <= MAX_NODES + 1
    else:
        assert cnt[0] == 0 and cnt[1] == 0


def test_add_mesh_equals_add_triangle():
    desc = scenes.soup_scene(129)
    V = tri_vertices(desc)
    # an indexed mesh that shares vertices: triangles over a small vertex pool, plus the soup's own vertices
    pool = V.reshape(-1, 3)
    g = scenes.Lcg(7)
    idx = np.array([[g.next_u32() % len(pool) for _ in range(3)] for _ in range(200)], np.uint32)
    m = Material(_lib.DIELECTRIC, Color(0.2, 0.7, 0.4), 0.6, 0.1)
    a, b = Scene(Color(1, 1, 1), 0.1), Scene(Color(1, 1, 1), 0.1)
    a.addSphere(Vector3(0, 1, 0), 1.0, m)
    b.addSphere(Vector3(0, 1, 0), 1.0, m)
    handles = a.addMesh(pool, idx, m)
    assert [h.obj for h in handles] == list(range(1, 201))
    for i in idx:
        b.addTriangle(Vector3(*pool[i[0]]), Vector3(*pool[i[1]]), Vector3(*pool[i[2]]), m)
    assert a.counts() == b.counts() == (1, 200, 0, 0)
    da, db = a.tri_bvh_dump(), b.tri_bvh_dump()
    assert da is not None
    for k in ("nodes", "leaves", "leaf_size", "depth"):
        assert da[k] == db[k]
    for k in ("boxes", "children", "leaf_ids", "residual"):
        assert np.array_equal(da[k], db[k]), k


def test_add_mesh_rejects_bad_index():
    s = Scene(Color(1, 1, 1), 0.1)
    v = np.zeros((3, 3), np.float32)
    with pytest.raises(_lib.RfxError):
        s.addMesh(v, np.array([[0, 1, 2], [0, 1, 3]], np.uint32), Material())
    assert s.counts()[1] == 0  # nothing was added
    assert len(s.addMesh(v, np.zeros((0, 3), np.uint32), Material())) == 0
