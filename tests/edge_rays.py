"""Shared by the edge-ray tests (test_edge_rays_host.py, test_bvh_prune_bound.py, test_gpu_edge_rays.py): rays a caller
may hand to rfx_trace_rays / rfx_query_hits / rfx_query_occluded that no pinhole frame or reflection produces -- zero
and -0.0 components, directions 1e-18 or 3e19 long, origins 1e5 scene sizes away, NaN and infinite words among good
lanes -- the `layers` scene, and the reference's answers for them (hits_helpers.compose, rays_helpers.oracle_trace).

Every family is a pure function of rays_helpers.incoherent_rays(name): `base` below is those 357 rays, `u` their
directions normalised in float64, `o` their origins; results are cast to float32 last.
"""
from __future__ import annotations

import numpy as np

from hits_helpers import compose
from rays_helpers import incoherent_rays, scene
from reflaxman_amd import scenes

LENGTHS = ("1e-9", "1e-18", "3e-19", "1e17", "1e19", "3e19", "1e20")
FARS = ("1e3", "1e5", "1e7")
NONFINITE_ROTATION = 37
# `mixed` takes ray i from FAMILIES[i % len(FAMILIES)]
FAMILIES = tuple("len_" + L for L in LENGTHS) + ("axis", "axis_pos") + tuple("far_" + D for D in FARS) + \
    ("nonfinite", "nonfinite_rot")
ALL = FAMILIES + ("mixed",)
# the scenes the GPU tests add to rays_helpers' take the rays of the scene they grew from
RAYS_OF = {"mesh100_plane": "mesh100"}
LAYERS_N = 256
LAYERS_LENGTHS = ("1", "1e-18", "3e-19", "1e19", "3e19")
_DESC, _FAM = {}, {}


def _unit(base):
    d = base[:, 3:6].astype(np.float64)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def nonfinite_of(good):
    """`good` with the family's three edits: for j, i in enumerate(range(0, n, 5)) word j % 6 of ray i becomes NaN,
    +inf or -inf; rays 3, 53, 103, ... get the zero direction.  Ray 0 is edited: a bad ray is wave 0's first lane."""
    rays = np.array(good, np.float32)
    vals = (np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf))
    for j, i in enumerate(range(0, len(rays), 5)):
        rays[i, j % 6] = vals[(j // 6) % 3]
    rays[3::50, 3:6] = 0.0
    return rays


def nonfinite_edited(n):
    """The rays nonfinite_of changes."""
    m = np.zeros(n, bool)
    m[0::5] = True
    m[3::50] = True
    return m


def family(name, fam):
    """(357, 6) float32: family `fam` of incoherent_rays(name)."""
    if (name, fam) in _FAM:
        return _FAM[(name, fam)]
    base = incoherent_rays(RAYS_OF.get(name, name))
    n = len(base)
    o, u = base[:, 0:3].astype(np.float64), _unit(base)
    if fam.startswith("len_"):
        rays = np.concatenate([o, u * float(fam[4:])], axis=1).astype(np.float32)
    elif fam in ("axis", "axis_pos"):
        rays = base.copy()
        for i in range(n):
            k = i % 7
            if k < 3:
                rays[i, 3 + k] = 0.0
            elif k < 6:
                rays[i, 3 + k - 3] = -0.0 if fam == "axis" else 0.0
                rays[i, 3 + (k - 2) % 3] = 0.0
    elif fam.startswith("far_"):
        rays = np.concatenate([o - u * float(fam[4:]), u], axis=1).astype(np.float32)
    elif fam == "nonfinite":
        rays = nonfinite_of(base)
    elif fam == "nonfinite_rot":  # the same rays, ray 37 first: lane 0 of wave 0 is a good ray
        rays = np.roll(family(name, "nonfinite"), -NONFINITE_ROTATION, axis=0)
    elif fam == "mixed":
        rays = np.stack([family(name, FAMILIES[i % len(FAMILIES)])[i] for i in range(n)])
    else:
        raise ValueError(fam)
    rays = np.ascontiguousarray(rays, np.float32)
    rays.setflags(write=False)
    _FAM[(name, fam)] = rays
    return rays


def oracle_ok(rays):
    """The rays rays_helpers.oracle_trace can carry: all words finite, no -0.0 direction component."""
    rays = np.asarray(rays, np.float32).reshape(-1, 6)
    d = rays[:, 3:6]
    return np.isfinite(rays).all(axis=1) & ~((d == 0) & np.signbit(d)).any(axis=1)


# ------------------------------------------------------------------ the `layers` scene
def layers_triangles():
    """The 48 triangles in geometric order (quad k = index // 2 at z = -6 + 0.5 k, corners alternately raised by
    0.125) and the order they are inserted in."""
    tris = []
    for k in range(24):
        z = -6.0 + 0.5 * k
        c = [(-3.0, -3.0, z), (3.0, -3.0, z + 0.125), (3.0, 3.0, z), (-3.0, 3.0, z + 0.125)]
        tris += [(c[0], c[1], c[2]), (c[0], c[2], c[3])]
    return tris, np.random.default_rng(5).permutation(48)


def layers_scene():
    """24 stacked quads along z, every ray of layers_rays crossing all of them: the closest hit is decided between
    24 candidates, met by a tree walk in an order that is neither the insertion order nor the distance order."""
    d = scenes.SceneDesc("layers", (0.9, 0.9, 1.0, 0.1), ((0.0, 0.0, -30.0), (0.0, 0.0, 0.0), 1.0))
    d.add_light((11.8e9, 4.26e9, 3.08e9), 3.48e8, (1.0, 1.0, 0.95), 0.85)
    tris, order = layers_triangles()
    for j in order:
        j = int(j)
        rgb = (0.2 + 0.8 * (j % 5) / 4.0, 0.2 + 0.8 * (j % 3) / 2.0, 0.2 + 0.8 * (j % 7) / 6.0)
        d.add_triangle(*tris[j], scenes.DIELECTRIC if j % 3 == 0 else scenes.METAL, rgb, 0.1 + 0.8 * (j % 4) / 3.0)
    return d


def layers_rays(L):
    """256 rays from z = +-30 (alternating) at points of the z = 0 plane, origins and targets uniform in
    [-2.5, 2.5]^2, directions of length float(L)."""
    key = ("layers", L)
    if key not in _FAM:
        g = np.random.default_rng(6)
        o = np.empty((LAYERS_N, 3))
        o[:, 0:2] = g.uniform(-2.5, 2.5, (LAYERS_N, 2))
        o[:, 2] = np.where(np.arange(LAYERS_N) % 2 == 0, 30.0, -30.0)
        t = np.zeros((LAYERS_N, 3))
        t[:, 0:2] = g.uniform(-2.5, 2.5, (LAYERS_N, 2))
        u = t - o
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        rays = np.concatenate([o, u * float(L)], axis=1).astype(np.float32)
        rays.setflags(write=False)
        _FAM[key] = rays
    return _FAM[key]


GRAZE_LENGTH = 1.31e19  # the shortest round length whose 2 |ray|^2 is +inf in float32 (|ray|^2 = 1.716e38 > FLT_MAX / 2)


def layers_graze():
    """256 rays of length 1.31e19 that cross the stack at 5 to 9 degrees to the quads, from 2 to 3 outside it: 114 of
    them cross two quads, 1.6 to 8 away.  Here 2 |ray|^2 is +inf while (normal . ray)^2 is not -- the operands
    of the closest-hit reject before the division (rfx_intersect.h tri_z), which must not take `+inf > finite` for
    `farther than the best hit`: the nearer crossing is often met second."""
    key = ("layers", "graze")
    if key not in _FAM:
        g = np.random.default_rng(7)
        n = LAYERS_N
        p = np.stack([g.uniform(-2.9, -2.0, n), g.uniform(-2.5, 2.5, n), g.uniform(-5.5, 5.5, n)], axis=1)
        s = g.uniform(0.08, 0.16, n) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        phi = g.uniform(-0.15, 0.15, n)
        c = np.sqrt(1.0 - s * s)
        u = np.stack([c * np.cos(phi), c * np.sin(phi), s], axis=1)
        o = p - u * g.uniform(2.0, 3.0, (n, 1))
        rays = np.concatenate([o, u * GRAZE_LENGTH], axis=1).astype(np.float32)
        rays.setflags(write=False)
        _FAM[key] = rays
    return _FAM[key]


def layers_far():
    """layers_rays("1") from 1e7 further back along each ray.  From there every crossing's distance lies within 2^-20
    (relative, squared) of every other's -- the band in which the closest-hit rule (rfx_intersect.h tri_takes) leaves
    its quick comparison for the exact one -- so nearly every candidate that takes does so inside the band."""
    key = ("layers", "far")
    if key not in _FAM:
        base = layers_rays("1")
        u = _unit(base)
        rays = np.concatenate([base[:, 0:3].astype(np.float64) - u * 1e7, u], axis=1).astype(np.float32)
        rays.setflags(write=False)
        _FAM[key] = rays
    return _FAM[key]


# ------------------------------------------------------------------ scenes, batches, references
def desc_of(name):
    """A scene description by name: rays_helpers' scenes, `layers`, and test_gpu_hits.py's mesh100_plane."""
    if name not in _DESC:
        if name == "layers":
            _DESC[name] = layers_scene()
        elif name == "mesh100_plane":  # a triangle tree and a plane in one scene
            d = scenes.get_scene("mesh100")
            d.add_plane((0.0, -0.05, 0.0), (0.0, 2.0, 0.0), scenes.DIELECTRIC, (0.8, 0.85, 0.9), 0.6)
            _DESC[name] = d
        else:
            _DESC[name] = scene(name)
    return _DESC[name]


def batches(name):
    """The names of the edge batches of a scene: every family and `mixed`, or -- `layers` -- its lengths, `graze` and `far`."""
    return tuple("L" + L for L in LAYERS_LENGTHS) + ("graze", "far") if name == "layers" else ALL


def batch(name, fam):
    if name == "layers":
        return layers_graze() if fam == "graze" else layers_far() if fam == "far" else layers_rays(fam[1:])
    return family(name, fam)


def composed(name, fam):
    """hits_helpers.compose on batch(name, fam), computed once: (closest-hit planes, table)."""
    return compose(desc_of(name), batch(name, fam), key=("edge", name, fam))


COLOUR_FAMILIES = ("len_1e-18", "len_1e19", "len_3e19", "axis_pos", "far_1e3", "far_1e7", "mixed")
_COLOURS = {}


def colour_batches(name):
    """The batches whose colours the 1 x 1 oracle can give: no -0.0, no non-finite word (of `mixed`: that part)."""
    return ("L1", "L1e-18", "L1e19", "L3e19", "graze", "far") if name == "layers" else COLOUR_FAMILIES


def colour_rays(name, fam):
    rays = batch(name, fam)
    return rays[oracle_ok(rays)]


def colours(name, fam, depth, seed):
    """(colours, the sphere stream's end state, the oracle's summed counters) of rays_helpers.oracle_trace on
    colour_rays(name, fam) -- computed once."""
    import oracle as orc
    from rays_helpers import oracle_trace
    key = (name, fam, depth, seed)
    if key not in _COLOURS:
        cnt = np.zeros(len(orc.COUNTER_NAMES), np.uint64)
        rgb, end = oracle_trace(desc_of(name), colour_rays(name, fam), depth, seed, cnt)
        rgb.setflags(write=False)
        cnt.setflags(write=False)
        _COLOURS[key] = (rgb, end, cnt)
    return _COLOURS[key]
