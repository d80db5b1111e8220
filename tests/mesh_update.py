"""What the moving-mesh tests share (tests/test_mesh_update_host.py, tests/test_gpu_mesh_update.py): scene
descriptions with their triangles moved, the vertex sets both files use, and the float32 replay of the kernel's box
test on boxes that are already widened."""
import copy

import numpy as np

from test_bvh_box_bound import F, K_CULL_REL, approx, fmaf

SEED = 1350490027


def tri_vertices(desc):
    """(triangles, 3, 3) float32, insertion order"""
    return np.array([[ob[1], ob[2], ob[3]] for ob in desc.objects if ob[0] == "triangle"], F)


def moved_desc(desc, V, first=0):
    """desc with triangles [first, first + len(V)) at the vertices V; everything else shared"""
    d = copy.copy(desc)
    d.objects = list(desc.objects)
    tri = [k for k, ob in enumerate(desc.objects) if ob[0] == "triangle"]
    for j, v in enumerate(np.asarray(V, F).reshape(-1, 3, 3)):
        k = tri[first + j]
        d.objects[k] = ("triangle", *(tuple(float(x) for x in p) for p in v), desc.objects[k][-1])
    d.name = desc.name + "_moved"
    return d


def wave(V, amp=0.25, phase=0.0):
    """a height wave on every vertex, a function of the vertex's (x, z) alone: shared vertices stay shared"""
    V = np.array(V, F)
    V[..., 1] += (amp * np.sin(0.9 * V[..., 0].astype(np.float64) + 0.7 * V[..., 2] + phase)).astype(F)
    return V


def pooled(V):
    """(pool (m, 3), indices (n, 3) uint32): the indexed form of the triangles V"""
    pool, inv = np.unique(np.asarray(V, F).reshape(-1, 3), axis=0, return_inverse=True)
    return np.ascontiguousarray(pool, F), np.ascontiguousarray(inv.reshape(-1, 3), np.uint32)


def special_triangles():
    """the triangles a vertex update can get wrong: huge, tiny, subnormal, a point, NaN and infinite vertices"""
    nan, inf = np.nan, np.inf
    return np.array([
        [(0, 0, 0), (1e30, 0, 0), (0, 1e30, 0)],
        [(1e15, 2e15, 0), (3e15, 0, 1e15), (0, 1e15, 2e15)],
        [(0, 0, 0), (1e-40, 0, 0), (0, 1e-40, 0)],
        [(1, 1, 1), (1 + 1e-6, 1, 1), (1, 1 + 1e-6, 1)],
        [(2, 3, 4), (2, 3, 4), (2, 3, 4)],
        [(nan, 0, 0), (1, 0, 0), (0, 1, 0)],
        [(0, 0, 0), (inf, 0, 0), (0, 1, 0)],
        [(0, 1, 0), (1, -inf, 0), (0, 0, nan)],
    ], F)


def case1_vertices():
    """300 triangles: 270 of the soup on a wave, then the 12 slivers (edge ratio 1e4), 2 zero-area triangles and 4 coincident
    pairs of scenes.degenerate_soup_scene, then special_triangles()"""
    from reflaxman_amd import scenes
    V = tri_vertices(scenes.degenerate_soup_scene())
    out = np.concatenate([wave(V[:270], amp=0.5), V[-22:], special_triangles()])
    assert out.shape == (300, 3, 3)
    return out


def kept_prewide(lo, hi, o, d, ref, rng):
    """rfx_bvh.h ray_inv + bvh_box for one child whose box (lo, hi) is the device copy, already widened by its node
    margin (tests/test_bvh_box_bound.py kept from its slab constants on)"""
    e = o - ref
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        dm = K_CULL_REL * (approx(np.sqrt((e * e).sum(1, dtype=F)), rng) * F(1.0001)) + F(1e-6)
        inv = np.fmin(np.fmax(approx(F(1) / d, rng), F(-1e30)), F(1e30))  # ray_inv's fin: a NaN becomes -1e30
        a = fmaf(lo, inv, -((o + dm[:, None]) * inv))
        b = fmaf(hi, inv, -((o - dm[:, None]) * inv))
        mn, mx = np.fmin(a, b), np.fmax(a, b)
        t0 = np.fmax(np.fmax(mn[:, 0], mn[:, 1]), np.fmax(mn[:, 2], F(0)))
        t1 = np.fmin(np.fmin(mx[:, 0], mx[:, 1]), mx[:, 2])
        return ~(t0 > t1 * F(1.00001) + F(1e-30)), t0, t1


def tree_paths(dump):
    """(triangles-with-a-leaf -> list of (node, child) from the root to its leaf) of a Scene.tri_bvh_dump()"""
    kids, ids = dump["children"], dump["leaf_ids"]
    up = {}
    for n in range(dump["nodes"]):
        for c in range(2):
            up[int(kids[n, c])] = (n, c)
    paths = {}
    for g in range(dump["leaves"]):
        p, k = [], ~g
        while k in up:
            p.append(up[k])
            k = up[k][0]
        assert k == 0
        for t in ids[g][ids[g] >= 0]:
            paths[int(t)] = p[::-1]
    return paths
