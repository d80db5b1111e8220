"""What the moving-mesh sequence tests share (tests/test_mesh_sequence_host.py, tests/test_gpu_mesh_sequences.py): a
model of a renderer's triangle state under updates, re-cuts, set_scene and order calls that uses no device, and the
fixed scripts both files run.

The model's state is (C, V): V the current vertices of every triangle, C the vertices at the last re-cut (None since the
last set_scene).  The expected tree is the host refit of the built tree at V while C is None, else the host mirror's cut
at C fitted to V; the expected records are those of a Scene built from the description and edited to V."""
import numpy as np

import recut_helpers as rh
from mesh_update import F, pooled, tri_vertices, wave
from reflaxman_amd import _lib
from test_gpu_mesh_update import built, desc_of, make_ill

T = _lib.RFX_ORDER_TILE
UPDATES = ("whole", "range", "indexed", "host_range")


class Op:
    """One operation of a script.  kind: whole / range / indexed / host_range (rows: the new vertices of triangles
    [first, first + len(rows)); dead: the triangles an indexed update leaves alone), recut, set_scene, order (n rays).
    check: a checkpoint of the device test's full check."""

    def __init__(self, kind, first=0, rows=None, dead=(), n=0, check=True):
        self.kind, self.first, self.dead, self.n, self.check = kind, int(first), tuple(int(t) for t in dead), int(n), check
        self.rows = None if rows is None else np.ascontiguousarray(rows, F).reshape(-1, 3, 3)
        assert (kind in UPDATES) == (rows is not None) and (not dead or kind == "indexed")

    def __repr__(self):
        if self.kind in UPDATES:
            return f"{self.kind}({self.first}, {len(self.rows)}{', dead=' + str(list(self.dead)) if self.dead else ''})"
        return f"order({self.n})" if self.kind == "order" else self.kind


def indexed_arrays(op):
    """(pool, indices) of an indexed update, through mesh_update.pooled; each triangle in op.dead names one index >= the
    pool size (which of its three, and how far past the end, follow its number)"""
    pool, idx = pooled(op.rows)
    for t in op.dead:
        idx[t - op.first, t % 3] = len(pool) + t % 5
    return pool, idx


class Model:
    def __init__(self, key):
        from reflaxman_amd.render import build_scene
        self.key, self.desc = key, desc_of(key)
        self.scene = built(key)[0]
        self.dump = self.scene.tri_bvh_dump()
        self.V0 = tri_vertices(self.desc)
        self.V0.setflags(write=False)
        self.n = len(self.V0)
        self.tree = rh.in_tree(self.dump, self.n)
        self.residual = np.sort(self.dump["residual"])
        # a triangle's object index: its place among the description's objects (build_scene adds them in that order)
        self.obj = np.array([k for k, ob in enumerate(self.desc.objects) if ob[0] == "triangle"], np.int32)
        self.edited = build_scene(self.desc)[0]
        self.C, self.V = None, self.V0.copy()

    def apply(self, op):
        a, b = op.first, op.first + (0 if op.rows is None else len(op.rows))
        if op.kind == "whole":
            assert (a, b) == (0, self.n)
            self.V = op.rows.copy()
        elif op.kind in ("range", "host_range"):
            self.V[a:b] = op.rows
        elif op.kind == "indexed":
            pool, idx = indexed_arrays(op)
            live = (idx < len(pool)).all(axis=1)
            assert (~live).sum() == len(op.dead)
            self.V[a:b][live] = pool[idx[live]]  # (what the device reads: the pool's copy of each vertex)
        elif op.kind == "recut":
            self.C = self.V.copy()
        elif op.kind == "set_scene":
            self.C, self.V = None, self.V0.copy()
        else:
            assert op.kind == "order"

    def expected(self):
        """dict of boxes, children, mt, leaf_ids, depth (the tree), records (the edited Scene's words) and ill"""
        if self.C is None:
            boxes, mt = self.scene.tri_bvh_refit(self.V, widen=True)
            out = {"boxes": boxes, "mt": mt, "children": self.dump["children"], "leaf_ids": self.dump["leaf_ids"],
                   "depth": self.dump["depth"]}
        else:
            r = self.scene.tri_bvh_recut(self.C, self.V, widen=True)
            out = {k: r[k] for k in ("boxes", "mt", "children", "leaf_ids", "depth")}
        self.edited.setTriangleVertices(0, self.V)
        out["records"] = self.edited.tri_records()
        out["ill"] = (out["records"][:, 28] == 0).astype(np.uint32)
        return out


def slots_of(leaf_ids, n):
    """slot[t]: the position of t in leaf_ids, -1 for a triangle that is not there"""
    flat = np.asarray(leaf_ids).reshape(-1)
    slot = np.full(n, -1, np.int32)
    at = np.flatnonzero(flat >= 0)
    slot[flat[at]] = at
    return slot


def order_rays(n, seed=31):
    """the n-ray batch of an order(n) operation: origins and targets through the scenes' box"""
    rng = np.random.default_rng(seed + n)
    o = rng.uniform((-14, 0.3, -12), (14, 9, 10), (n, 3))
    q = rng.uniform((-12, 0.0, -9), (12, 5, 9), (n, 3))
    return np.concatenate([o, q - o], axis=1).astype(F)


# ------------------------------------------------------------------------------------------------ the scripts
_BASE = {}


def base(key):
    """(V0, the built tree's dump) of a scene"""
    if key not in _BASE:
        m = Model(key)
        _BASE[key] = (m.V0, m.dump)
    return _BASE[key]


def partial_updates():
    """1. partial, indexed, dead-index and host-form updates on a re-cut tree (mesh: 384 triangles, all in the tree)"""
    V0, _ = base("mesh")
    S = rh.shuffle(V0)
    W = (wave(S, amp=0.6, phase=0.5) + F(0.05)).astype(F)
    last = wave(rh.shuffle(V0, amp=3.0, seed=7), amp=0.5)
    return "mesh", [Op("whole", 0, S), Op("recut"), Op("range", 10, W[10:33]),
                    Op("indexed", 40, W[40:49], dead=[44]), Op("host_range", 383, W[383:384]), Op("recut"),
                    Op("indexed", 0, last)]


def class_changes():
    """2. classes around a re-cut (soup300): six in-tree triangles turn ill, three turn well again in their leaves, a
    re-cut places them, two others turn ill under the re-cut tree.  Returns the six, the three and the two as well."""
    V0, dump = base("soup300")
    ids = dump["leaf_ids"]
    six = [int(t) for t in ids[[0, 3, 17, 30, 41, 55], 0]]
    two = [int(t) for t in ids[[8, 50], 1]]
    assert min(six + two) >= 0 and len(set(six + two)) == 8
    S = rh.shuffle(V0)
    A = make_ill(S, six)
    three = sorted(six)[-3:]  # the last leaf's two and one of the leaf before (the ill gather in index order)
    B = A.copy()
    B[three] = S[three]
    D = make_ill(B, two)
    ops = [Op("whole", 0, A), Op("recut"), Op("range", three[0], B[three[0]:three[-1] + 1]), Op("recut"),
           Op("indexed", min(two), D[min(two):max(two) + 1]), Op("recut")]
    return "soup300", ops, six, three, two


def set_scene_after_a_recut(key="mesh"):
    """3. set_scene after a re-cut (mesh): the built tree, its slots and depth come back, and updates and a re-cut go on.
    The mesh's built tree has the cut's depth and by-height shape, so a set_scene that kept the cut's would not show
    there: the same script also runs on `degenerate` (built depth 8, cut depth 7)."""
    V0, _ = base(key)
    W = (wave(V0, amp=0.6, phase=0.5) + F(0.05)).astype(F)
    return key, [Op("whole", 0, rh.shuffle(V0, seed=23)), Op("recut"), Op("set_scene"),
                    Op("range", 10, W[10:33]), Op("recut")]


def shared_sort_scratch():
    """4. order calls and re-cuts in turn (mesh: 384 in the tree, so the re-cut's count differs from the batches' both
    ways).  The two whole updates are there so that each re-cut has something new to cut."""
    V0, _ = base("mesh")
    return "mesh", [Op("whole", 0, rh.shuffle(V0), check=False), Op("order", n=3 * T + 5, check=False), Op("recut"),
                    Op("order", n=65, check=False), Op("whole", 0, wave(rh.shuffle(V0, amp=3.0, seed=7), amp=0.5), check=False),
                    Op("recut"), Op("order", n=3 * T + 5)]


# Seeds of the walks, chosen among 1..39: most of those meet tests/test_mesh_sequence_host.py's conditions (two re-cuts,
# a dead lane, an update that touches a residual triangle -- the last 22 of the 324 --, an update that changes a class);
# these two also draw every kind of operation, and 32 ends on a set_scene that directly follows a re-cut.
WALK_SEEDS = (13, 32)


def walk(seed, length=16):
    """5. a seeded walk on `degenerate` (324 triangles, 14 residual): operations, ranges, vertex sets and dead lanes
    drawn with numpy.random.default_rng(seed); every fifth operation a re-cut.  Ill triangles are slivers and zero-area
    ones (make_ill's first five)."""
    V0, _ = base("degenerate")
    n = len(V0)
    rng = np.random.default_rng(seed)
    ops = []
    for k in range(length):
        check = k % 4 == 3 or k == length - 1
        if k % 5 == 4:
            ops.append(Op("recut", check=check))
            continue
        kind = str(rng.choice(["whole", "range", "indexed", "host_range", "set_scene", "order"],
                              p=[0.15, 0.25, 0.3, 0.15, 0.05, 0.1]))
        if kind == "set_scene":
            ops.append(Op("set_scene", check=check))
            continue
        if kind == "order":
            ops.append(Op("order", n=int(rng.choice([65, 700, T + 1])), check=check))
            continue
        X = wave(rh.shuffle(V0, amp=float(rng.uniform(1.0, 5.0)), seed=int(rng.integers(1 << 30))),
                 amp=float(rng.uniform(0.1, 0.8)), phase=float(rng.uniform(0.0, 6.0)))
        if rng.random() < 0.5:
            X = make_ill(X, [int(t) for t in rng.choice(n, 5, replace=False)])
        if kind == "whole":
            ops.append(Op("whole", 0, X, check=check))
            continue
        count = int(rng.integers(1, 120))
        first = int(rng.integers(0, n - count + 1))
        dead = ()
        if kind == "indexed" and count >= 4:
            dead = sorted(int(t) for t in first + rng.choice(count, int(rng.integers(0, 3)), replace=False))
        ops.append(Op(kind, first, X[first:first + count], dead=dead, check=check))
    return "degenerate", ops
