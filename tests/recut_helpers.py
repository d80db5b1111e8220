"""What the re-cut tests share (tests/test_tri_recut_host.py, tests/test_gpu_tri_recut.py): a numpy float32 restatement
of rfx.h "Re-cutting" steps 1-5, the builder's box formula in float64, the vertex sets both files cut at, and the
edge- and vertex-aimed rays of the moving-mesh host test."""
import numpy as np

from mesh_update import F
from test_gpu_mesh_update import make_ill  # noqa: F401 (the moving-mesh device tests' recipe, for both files)

LEAF = 4
LAST_KEY = 0x40000000
NAN_WORD = 0x7FC00000
K_WIDEN = 2e-3  # rfx_refit.h bvh_child_set: the node part of the cull margin


def shuffle(V, amp=6.0, seed=11):
    """every triangle moved as a whole by its own offset in [-amp, amp)^3: the mesh leaves the shape its tree was cut at"""
    rng = np.random.default_rng(seed)
    V = np.asarray(V, F)
    return (V + rng.uniform(-amp, amp, (len(V), 1, 3)).astype(F)).astype(F)


def classes(scene_like, V):
    """ill[t] of every triangle at the vertices V, as the library classes them (word [28] of the records, inverted)"""
    from reflaxman_amd.render import build_scene
    s, _ = build_scene(scene_like)
    s.setTriangleVertices(0, V)
    return (s.tri_records()[:, 28] == 0).astype(np.uint32)


def in_tree(dump, n_tri):
    """the in-tree triangles of a Scene.tri_bvh_dump(), ascending"""
    t = np.ones(n_tri, bool)
    t[dump["residual"]] = False
    ids = dump["leaf_ids"]
    assert np.array_equal(np.sort(ids[ids >= 0]), np.flatnonzero(t))
    return np.flatnonzero(t).astype(np.int32)


def cut_keys(V, ill):
    """steps 1-3 on the in-tree triangles' vertices V (T, 3, 3) float32 and class flags: (keys, placed, lo, hi, scale)"""
    V = np.asarray(V, F)
    with np.errstate(invalid="ignore", over="ignore"):
        s = (V[:, 0, :] + V[:, 1, :]) + V[:, 2, :]
        assert s.dtype == F
        placed = (np.asarray(ill) == 0) & np.isfinite(s).all(axis=1)
        keys = np.full(len(V), LAST_KEY, np.uint32)
        if not placed.any():
            return keys, placed, None, None, F(0)
        lo, hi = s[placed].min(axis=0), s[placed].max(axis=0)
        e = (hi - lo).max()
        scale = F(1024) / e if np.isfinite(e) and e > 0 else F(0)
        q = np.fmin(np.fmax((s[placed] - lo) * scale, F(0)), F(1023)).astype(np.uint32)
    k = np.zeros(len(q), np.uint32)
    for b in range(10):
        for a in range(3):
            k |= ((q[:, a] >> np.uint32(b)) & np.uint32(1)) << np.uint32(3 * b + a)
    keys[placed] = k
    return keys, placed, lo, hi, scale


def cut_topology(G):
    """step 5: (children (G - 1, 2) int32, depth) of the leaf count alone"""
    kids = []

    def node(a, b, level):
        if b - a == 1:
            return ~a, level
        i = len(kids)
        kids.append([0, 0])
        mid = a + (b - a) // 2
        l, dl = node(a, mid, level + 1)
        r, dr = node(mid, b, level + 1)
        kids[i] = [l, r]
        return i, max(dl, dr)

    _, depth = node(0, G, 0)
    return np.array(kids, np.int32).reshape(-1, 2), depth


def restated(V_all, ill_all, tree):
    """steps 1-5 from every triangle's cut vertices and class flags and the in-tree list: dict of leaf_ids (G, 4),
    children, depth, keys (in the tree list's order) and placed"""
    keys, placed, lo, hi, scale = cut_keys(np.asarray(V_all, F)[tree], np.asarray(ill_all)[tree])
    order = tree[np.argsort(keys, kind="stable")]
    G = (len(tree) + LEAF - 1) // LEAF
    ids = np.full(G * LEAF, -1, np.int32)
    ids[:len(order)] = order
    kids, depth = cut_topology(G)
    assert depth == (G - 1).bit_length()
    return {"leaf_ids": ids.reshape(G, LEAF), "children": kids, "depth": depth, "keys": keys, "placed": placed,
            "lo": lo, "hi": hi, "scale": scale}


def ref_point(V_built, residual):
    """rfx_scene.cpp tri_ref_point: the centre of the built scene's well-conditioned triangles' vertex box (scenes with
    at most 32 spheres)"""
    well = np.ones(len(V_built), bool)
    well[residual] = False
    pts = np.asarray(V_built, F)[well].reshape(-1, 3).astype(np.float64)
    return (0.5 * (pts.min(0) + pts.max(0))).astype(F)


def up(x):
    return np.nextafter(F(x), F(np.inf))


def down(x):
    return np.nextafter(F(x), F(-np.inf))


def child_box(lo, hi, ref, widen):
    """rfx_refit.h bvh_child_set in float64, operation for operation: (six bounds, mt) as float32"""
    l, h, ref = np.array(lo, np.float64), np.array(hi, np.float64), np.asarray(ref, np.float64)

    def terms():
        cd = hd = 0.0
        for k in range(3):
            dc, dh = ref[k] - 0.5 * (l[k] + h[k]), 0.5 * (h[k] - l[k])
            cd += dc * dc
            hd += dh * dh
        return np.sqrt(cd) + np.sqrt(hd)

    if widen:
        w = K_WIDEN * np.float64(up(F(terms() * 1.0001))) * (1.0 + 1e-6)
        l, h = l - w, h + w
    box = np.array([down(F(x)) for x in l] + [up(F(x)) for x in h], F)
    return box, up(F(terms() * 1.0001))


def fitted(ids, kids, V_all, ill_all, ref, widen):
    """the refit's boxes on a topology: (boxes (nodes, 2, 6), mt (nodes, 2)); NaN bounds and an infinite margin term
    above a leaf that holds an ill triangle"""
    V_all = np.asarray(V_all, F)
    G = len(ids)
    leaf = []
    for g in range(G):
        t = ids[g][ids[g] >= 0]
        with np.errstate(invalid="ignore"):
            v = V_all[t].reshape(-1, 3)
            leaf.append((np.fmin.reduce(v, axis=0), np.fmax.reduce(v, axis=0), bool(np.asarray(ill_all)[t].any())))
    boxes, mt = np.zeros((len(kids), 2, 6), F), np.zeros((len(kids), 2), F)

    def below(c):
        if c < 0:
            return leaf[~c]
        out = None
        for k in range(2):
            lo, hi, ill = below(int(kids[c, k]))
            if ill:
                boxes[c, k], mt[c, k] = np.uint32(NAN_WORD).view(F), np.inf
            else:
                boxes[c, k], mt[c, k] = child_box(lo, hi, ref, widen)
            out = (lo, hi, ill) if out is None else (np.fmin(out[0], lo), np.fmax(out[1], hi), out[2] or ill)
        return out

    below(0)
    return boxes, mt


def words(a):
    """float arrays as words, every NaN canonical"""
    w = np.ascontiguousarray(a, F).view(np.uint32).copy()
    w[np.isnan(np.asarray(a, F))] = NAN_WORD
    return w


def edge_rays(V, tree, extra, n=1 << 16, seed=1350490027):
    """tests/test_mesh_update_host.py's rays: n rays aimed near the edges and vertices of in-tree triangles of V (every
    16th at one of `extra`), from 0.05 to 2000 triangle sizes away: (kat records (n, 21), the target triangles, rng)"""
    rng = np.random.default_rng(seed)
    t = np.asarray(tree, np.int64)[rng.integers(0, len(tree), n)]
    t[::16] = np.asarray(extra)[rng.integers(0, len(extra), len(t[::16]))]
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
    return rec, t, rng
