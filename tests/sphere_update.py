"""What the moving-sphere tests share (tests/test_sphere_update_host.py, tests/test_gpu_sphere_update.py): scene
descriptions with their spheres moved, the sphere sets both files use, the record words restated in numpy, and the pair
tree's paths and reference point."""
import copy

import numpy as np

from mesh_update import F, SEED, tree_paths  # noqa: F401  (re-exported)

K_VERY_SMALL = F(1.0842021724855044e-19)  # rfx_math.h kVerySmall (the reference's VERY_SMALL_NUMBER)
NAN_WORD = np.uint32(0x7FC00000)


def sph_data(desc):
    """(spheres, 4) float32, insertion order: centre, radius as the description has it"""
    return np.array([[*ob[1], ob[2]] for ob in desc.objects if ob[0] == "sphere"], F).reshape(-1, 4)


def moved_desc(desc, S, ids=None, first=0):
    """desc with spheres [first, first + len(S)) -- or the spheres `ids` -- at the centres and radii S; the rest shared"""
    d = copy.copy(desc)
    d.objects = list(desc.objects)
    sph = [k for k, ob in enumerate(desc.objects) if ob[0] == "sphere"]
    S = np.asarray(S, F).reshape(-1, 4)
    which = range(first, first + len(S)) if ids is None else ids
    for j, i in enumerate(which):
        if i >= len(sph):
            continue
        k = sph[i]
        d.objects[k] = ("sphere", tuple(float(x) for x in S[j, :3]), float(S[j, 3]), desc.objects[k][-1])
    d.name = desc.name + "_moved"
    return d


def jiggle(S, seed=11):
    """centres +- 0.3, radii x [0.8, 1.25]"""
    rng = np.random.default_rng(seed)
    out = np.array(S, F)
    out[:, :3] += rng.uniform(-0.3, 0.3, (len(out), 3)).astype(F)
    out[:, 3] *= rng.uniform(0.8, 1.25, len(out)).astype(F)
    return out


def shuffle(S, seed=12):
    """the centres permuted among the spheres (the radii stay): the tree's topology is stale everywhere"""
    rng = np.random.default_rng(seed)
    out = np.array(S, F)
    out[:, :3] = out[rng.permutation(len(out)), :3]
    return out


def clamped(S):
    """the radii as the constructor leaves them (Sphere.cpp:13-19): a NaN passes"""
    out = np.array(S, F)
    r = out[:, 3]
    out[:, 3] = np.where(r <= K_VERY_SMALL, K_VERY_SMALL, r)
    return out


def canonical(words):
    w = np.array(words, copy=True).view(np.uint32)
    w[(w & 0x7FFFFFFF) > 0x7F800000] = NAN_WORD
    return w


def record_words(S):
    """rfx.h RFX_SPH_RECORD_WORDS per sphere, restated: (centre, r r), the same again, (centre, r 1.00001f)"""
    c = clamped(S)
    with np.errstate(over="ignore", invalid="ignore"):
        r2 = (c[:, 3] * c[:, 3]).astype(F)
        rb = (c[:, 3] * F(1.00001)).astype(F)
    geo = np.concatenate([c[:, :3], r2[:, None]], axis=1)
    return canonical(np.concatenate([geo, geo, c[:, :3], rb[:, None]], axis=1).astype(F))


def sphere_boxes(S):
    """each sphere's own box c -+ (double)(r 1.00001f): (lo (n, 3), hi (n, 3)) float64"""
    c = clamped(S)
    with np.errstate(over="ignore", invalid="ignore"):
        rb = (c[:, 3] * F(1.00001)).astype(F).astype(np.float64)
        cc = c[:, :3].astype(np.float64)
        return cc - rb[:, None], cc + rb[:, None]


def ref_point(S_built):
    """the pair tree's margin reference point of a scene built at S_built: the root box centre as a float
    (rfx_scene.cpp sphere_bvh)"""
    lo, hi = sphere_boxes(S_built)
    return (0.5 * (np.nanmin(lo, axis=0) + np.nanmax(hi, axis=0))).astype(F)


def special_spheres(camera_eye):
    """the spheres an update can get wrong: (k, 4) -- radius 0, -1, 1e-30, NaN, +inf; a NaN and an infinite centre
    component; centre 1e30; centre 1e15 with radius 1e14; one enclosing the camera; two coincident"""
    nan, inf = np.nan, np.inf
    ex, ey, ez = camera_eye
    return np.array([
        (1.0, 1.0, 2.0, 0.0),
        (-2.0, 1.0, 1.0, -1.0),
        (3.0, 0.5, -1.0, 1e-30),
        (0.0, 2.0, 0.0, nan),
        (4.0, 1.0, 3.0, inf),
        (nan, 1.0, 2.0, 0.7),
        (2.0, inf, -2.0, 0.6),
        (1e30, 0.0, 1.0, 1.0),
        (1e15, 2e15, -1e15, 1e14),
        (ex, ey, ez, 3.0),
        (-3.0, 1.2, 2.5, 0.8),
        (-3.0, 1.2, 2.5, 0.8),
    ], F)


# of special_spheres: the infinite radius and the infinite centre component.  The first makes its leaf's box (-inf, +inf)
# and the builder's widening NaN (inf - inf): all of space, kept by every ray.  The second makes one bound infinite, the
# widening infinite and so all six bounds of every child above it infinite: kept by every ray whose slab constants are
# finite, lost where one overflows (DESIGN.md "Moving spheres -> Spheres that are not finite").
INFINITE_RADIUS, INFINITE_CENTRE = 4, 6
