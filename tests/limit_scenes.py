"""What the tree-limit tests share (tests/test_tree_limits_host.py, tests/test_gpu_tree_limits.py; no device): scenes with
exactly as many spheres or triangles as the largest hierarchy the walkers' int16 stack slots can take (rfx_bvh.h BvhSlot:
32,767 nodes, 32,768 leaves) and one primitive more, the rays aimed at the leaves where an off-by-one would show, and the
reference's answers composed with the object axis taken in blocks.  Every description, built Scene and composed answer is
made once per process and never edited."""
import copy
from bisect import bisect_left
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from hits_helpers import FLT_MAX, table
from reflaxman_amd import _lib, scenes
from span_helpers import eligible

F = np.float32
LIMIT_LEAVES = 32768  # the last leaf is ~32767 = INT16_MIN; one node fewer
N_RAYS = 128          # scene rays, and as many aimed ones
AIM_FROM = 1.25       # an aimed ray starts this many radii from its sphere's centre
_RAW, _DESC, _BUILT, _RAYS, _COMPOSED = [], {}, {}, {}, {}


def switches():
    """(spheres a pair-tree leaf holds, triangles a triangle-tree leaf holds) of the loaded library: rfx_build_options'
    pairs a leaf, and the leaf size a small mesh's triangle-tree dump reports"""
    if "switches" not in _BUILT:
        from reflaxman_amd.render import build_scene
        leaf = build_scene(scenes.mesh_scene(16, 12))[0].tri_bvh_dump()["leaf_size"]
        _BUILT["switches"] = (2 * ((_lib.load().rfx_build_options() >> 8) & 0xFF), int(leaf))
    return _BUILT["switches"]


def n_s():
    return switches()[0] * LIMIT_LEAVES


def n_t():
    return switches()[1] * LIMIT_LEAVES


# ------------------------------------------------------------------------------------------------ descriptions
def _raw(n):
    """the first n draws of scenes._lcg_spheres (same generator, same draw order), kept between calls"""
    if not _RAW:
        _RAW.append((scenes.Lcg(20261015), []))
    g, rows = _RAW[0]
    while len(rows) < n:
        r = g.uniform(0.1, 0.6)
        x = g.uniform(-12.0, 12.0)
        z = g.uniform(-9.0, 9.0)
        mt = scenes.DIELECTRIC if (g.next_u32() >> 31) else scenes.METAL
        rgb = (g.uniform(0, 1), g.uniform(0, 1), g.uniform(0, 1))
        rows.append((r, x, z, mt, rgb, g.uniform(0, 1)))
    return rows[:n]


def spheres_at(n):
    """scenes.stress_scene(n) with every radius scaled by sqrt(4096 / n): the ground stays as densely covered as
    stress4096's whatever n is (at the generator's own radii 262,144 spheres overlap some 200 deep, the tree prunes
    nothing and every ray ties)"""
    key = ("spheres", n)
    if key not in _DESC:
        s = scenes._base(f"limit_spheres{n}")
        scenes._add_sun(s)
        k = float(np.sqrt(4096.0 / n))
        for (r, x, z, mt, rgb, refl) in _raw(n):
            s.add_sphere((x, r * k, z), r * k, mt, rgb, refl)
        scenes._add_ground(s, s.add_texture(scenes.Texture("himiya", None)))
        _DESC[key] = s
    return _DESC[key]


def mesh_at(extra):
    """scenes.mesh_scene's height field with n_t() triangles (256 x 256 cells at four triangles a leaf), plus `extra`
    well-conditioned triangles floating above it, in the camera's view"""
    key = ("mesh", extra)
    if key not in _DESC:
        if ("mesh", 0) not in _DESC:
            _DESC[("mesh", 0)] = scenes.mesh_scene(n_t() // 512, 256)
            assert _DESC[("mesh", 0)].n_triangles == n_t()
        s = _DESC[("mesh", 0)]
        if extra:
            s = copy.copy(s)
            s.objects, s.settex = list(s.objects), list(s.settex)
            s.name += f"_plus{extra}"
            for k in range(extra):  # (five units in front of the default camera, facing it, one beside the other)
                z = -2.3 + 1.6 * k
                s.add_triangle((3.3, 1.2, z), (3.3, 2.3, z + 0.6), (3.0, 1.3, z + 1.3), scenes.METAL, (0.9, 0.4, 0.2), 0.5)
        _DESC[key] = s
    return _DESC[key]


CASES = {"S_max": lambda: spheres_at(n_s()), "S_over": lambda: spheres_at(n_s() + 1),
         "T_max": lambda: mesh_at(0), "T_over": lambda: mesh_at(1)}


def desc_of(case):
    return CASES[case]()


def built(case):
    """(Scene, Camera, dump) of a case -- the pair tree's dump for the sphere cases, the triangle tree's (None without a
    tree) for the mesh cases"""
    if case not in _BUILT:
        from reflaxman_amd.render import build_scene
        s, cam = build_scene(desc_of(case))
        _BUILT[case] = (s, cam, s.sph_bvh_dump() if case[0] == "S" else s.tri_bvh_dump())
    return _BUILT[case]


# ------------------------------------------------------------------------------------------------ the tree's far corners
def last_node_leaves(dump):
    """the leaves below the last node (its children that are leaves, and the leaves of those that are nodes)"""
    kids, todo, out = dump["children"], [dump["nodes"] - 1], []
    while todo:
        for c in kids[todo.pop()]:
            (out if c < 0 else todo).append(int(~c) if c < 0 else int(c))
    return sorted(out)


def leaf_prims(dump, leaf):
    ids = dump["leaf_ids"][leaf]
    return [int(i) for i in ids[ids >= 0]]


def targets(case):
    """(primitive index of every aimed ray (N_RAYS,), {"first", "last", "under_last_node"} -> the primitives of those
    leaves) -- the primitives of leaf 0, of the last leaf and of the leaves under the last node, then one primitive
    each of leaves drawn with a fixed seed; the no-tree cases take their tree's targets (the same primitive numbers)"""
    _, _, d = built(case[0] + "_max")
    named = {"first": leaf_prims(d, 0), "last": leaf_prims(d, d["leaves"] - 1),
             "under_last_node": [p for g in last_node_leaves(d) for p in leaf_prims(d, g)]}
    out = []
    for p in named["first"] + named["last"] + named["under_last_node"]:
        if p not in out:
            out.append(p)
    rng = np.random.default_rng(26)
    for g in rng.permutation(d["leaves"]):
        if len(out) == N_RAYS:
            break
        p = leaf_prims(d, int(g))[0]
        if p not in out:
            out.append(p)
    return np.array(out), named


def sphere_rows(desc):
    return np.array([[*ob[1], ob[2]] for ob in desc.objects if ob[0] == "sphere"], F).reshape(-1, 4)


def triangle_rows(desc):
    return np.array([[ob[1], ob[2], ob[3]] for ob in desc.objects if ob[0] == "triangle"], F)


def prim_objects(desc, kind):
    """object index of every sphere (or triangle) of desc, insertion order"""
    return np.array([k for k, ob in enumerate(desc.objects) if ob[0] == kind])


def rays_of(case):
    """(2 N_RAYS, 6) float32: N_RAYS drawn as test_gpu_mesh_update.rays_at_the_scene draws them, then the aimed ones --
    from AIM_FROM r off a sphere's centre in a direction of the upper half space, or from 0.05 above a triangle's centroid
    along its upward normal, at the centre"""
    if case not in _RAYS:
        rng = np.random.default_rng(5)
        o = rng.uniform((-14, 0.3, -12), (14, 9, 10), (N_RAYS, 3))
        q = rng.uniform((-12, 0.0, -9), (12, 5, 9), (N_RAYS, 3))
        scene_rays = np.concatenate([o, (q - o) * rng.uniform(0.2, 3.0, (N_RAYS, 1))], axis=1)
        prims, _ = targets(case)
        desc = desc_of(case)
        if case[0] == "S":
            S = sphere_rows(desc)[prims].astype(np.float64)
            u = np.random.default_rng(7).normal(size=(N_RAYS, 3))
            u[:, 1] = np.abs(u[:, 1]) + 1.0
            u /= np.linalg.norm(u, axis=1)[:, None]
            start = S[:, :3] + AIM_FROM * S[:, 3:4] * u
            aimed = np.concatenate([start, S[:, :3] - start], axis=1)
        else:
            V = triangle_rows(desc)[prims].astype(np.float64)
            c = V.mean(axis=1)
            nrm = np.cross(V[:, 1] - V[:, 0], V[:, 2] - V[:, 0])
            nrm *= (np.where(nrm[:, 1] < 0, -1.0, 1.0) / np.linalg.norm(nrm, axis=1))[:, None]
            start = c + 0.05 * nrm
            aimed = np.concatenate([start, c - start], axis=1)
        rays = np.concatenate([scene_rays, aimed]).astype(F)
        # (what rays_helpers.oracle_trace can carry: finite words, no -0.0 direction component)
        assert np.isfinite(rays).all() and not ((rays[:, 3:6] == 0) & np.signbit(rays[:, 3:6])).any()
        rays.setflags(write=False)
        _RAYS[case] = rays
    return _RAYS[case]


# ------------------------------------------------------------------------------------------------ the reference, in blocks
class _Block:
    """objects [b0, b1) of a description and the settex entries that name them, as hits_helpers.table reads one"""

    def __init__(self, desc, b0, b1, settex):
        self.objects, self.textures = desc.objects[b0:b1], desc.textures
        self.settex = [(oi - b0, ti, uv) for (oi, ti, uv) in settex]


def compose_blocked(desc, rays, block=4096, lo=None, after=None, hi=None, skip=None):
    """(closest-hit planes, any-hit flags) of hits_helpers.compose -- closest(table) and any_hit(table, skip) -- with the
    object axis taken `block` objects at a time (the whole table of 262,144 objects x 256 rays is 4 GB).  The running
    closest hit is replaced on a strictly smaller distance only, blocks in insertion order: np.argmin's first minimum.
    lo / after / hi: span_helpers' interval, applied to both answers (closest_span, any_hit_span)."""
    rays = np.ascontiguousarray(rays, F).reshape(-1, 6)
    n, m = len(rays), len(desc.objects)
    ar = np.arange(n)
    best = np.full(n, np.inf, F)
    win = np.zeros(n, np.int64)
    rec, col = np.zeros((n, 15), F), np.zeros((n, 3), F)
    occ = np.zeros(n, bool)
    skip = None if skip is None else np.broadcast_to(np.asarray(skip, np.int64), (n,))
    span = lo is not None or hi is not None
    settex = sorted(desc.settex)
    first = [oi for (oi, _, _) in settex]

    def one(b0):
        """block [b0, b1)'s own answer: (distances, winners, their records and colours, any-hit flags)"""
        b1 = min(m, b0 + block)
        tab, tcol = table(_Block(desc, b0, b1, settex[bisect_left(first, b0):bisect_left(first, b1)]), rays)
        ok = tab[:, :, 0] > 0
        flags = tab[:, :, 14] > 0
        if span:
            af = None if after is None else np.asarray(after, np.int64) - b0
            ok = eligible(tab, lo, af, hi)
            flags = eligible(tab, lo, None, hi)  # (any_hit_span reads the out-parameter form's candidates)
        dist = np.where(ok, tab[:, :, 10], F(np.inf))
        w = np.argmin(dist, axis=0)
        if skip is not None:
            here = (skip >= b0) & (skip < b1)
            flags = flags.copy()
            flags[skip[here] - b0, ar[here]] = False
        return dist[w, ar], w + b0, tab[w, ar], tcol[w, ar], flags.any(axis=0)

    # (the known-answer entries run outside the interpreter's lock: blocks in parallel, merged in insertion order)
    with ThreadPoolExecutor(max_workers=8) as pool:
        for d, w, r, c, o in pool.map(one, range(0, m, block)):
            take = d < best
            best[take], win[take], rec[take], col[take] = d[take], w[take], r[take], c[take]
            occ |= o
    hit = np.isfinite(best)
    z3, h3 = np.zeros((n, 3), F), hit[:, None]
    planes = {"object": np.where(hit, win, -1).astype(np.int32), "distance": np.where(hit, rec[:, 10], FLT_MAX).astype(F),
              "point": np.where(h3, rec[:, 1:4], z3), "normal": np.where(h3, rec[:, 4:7], z3),
              "reflected": np.where(h3, rec[:, 7:10], z3), "colour": np.where(h3, col, z3)}
    return planes, occ.astype(np.uint8)


def composed(case, layer=0):
    """compose_blocked on rays_of(case), once: layer 0 the closest hits and any-hit flags, layer 1 the next hits behind
    them (lo = layer 0's distance, +inf on a miss; after = its object)"""
    key = (case, layer)
    if key not in _COMPOSED:
        kw = {}
        if layer:
            first = composed(case)[0]
            kw = {"lo": np.where(first["object"] < 0, F(np.inf), first["distance"]), "after": first["object"]}
        res = compose_blocked(desc_of(case), rays_of(case), **kw)
        for a in list(res[0].values()) + [res[1]]:
            a.setflags(write=False)
        _COMPOSED[key] = res
    return _COMPOSED[key]
