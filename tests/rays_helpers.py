"""Shared by the ray-batch tests (test_gpu_rays.py, test_rays_host.py): the per-ray oracle and the fixed test rays.

The oracle for an arbitrary ray is oracle.OracleRender at image size 1 x 1, which traces exactly one Scene::trace: with
eye = origin and view = (-2dx, 0, 0, -2dy, 0, 0, -2dz, 0, 0) its one ray is (-2d)(-0.5) + 0 + 0 = d exactly, whatever
the fov (Render.cpp:146-156, 184-185), and its sphere stream carries on from ray to ray as the reference's would.  A
+0.0 direction component survives the trick ((-2 * 0)(-0.5) + 0 + 0 = +0.0), a -0.0 one comes out as +0.0, and a
non-finite word cannot be carried: oracle_trace takes finite rays without -0.0 components (the fixed test rays below
hold no zero components at all; tests/edge_rays.py derives the ones that do).
"""
from __future__ import annotations

import numpy as np

import oracle as orc
from reflaxman_amd import scenes

NRAYS = 357   # five full waves plus 37
SEED = 4242
DEPTH = 8
_SCENES, _RAYS, _ORACLE = {}, {}, {}


def scene(name):
    if name not in _SCENES:
        _SCENES[name] = scenes.get_scene(name)
    return _SCENES[name]


def oracle_trace(desc, rays, depth, seed, counters=None):
    """n consecutive Scene::trace(origin_i, ray_i, depth) from sphere-stream state `seed`: ((n, 3) float32 colours,
    the state after them).  counters: the oracle's event counters are added to it."""
    rays = np.asarray(rays, np.float32).reshape(-1, 6)
    assert np.isfinite(rays).all() and not ((rays[:, 3:6] == 0) & np.signbit(rays[:, 3:6])).any(), \
        "the 1 x 1 oracle cannot carry a non-finite word or a -0.0 direction component"
    o = orc.OracleRender(desc, seed, 0)
    o.set_image_size(1, 1)
    out = np.empty((rays.shape[0], 3), np.float32)
    for i, r in enumerate(rays):
        o.scene.eye = np.array(r[0:3], np.float32)
        v = np.zeros(9, np.float32)
        v[0::3] = np.float32(-2.0) * r[3:6]
        o.scene.view = v
        o.render(depth, 1, counters=counters)
        out[i] = o.image[0, 0]
    return out, o.sphere_seed.value


def scene_box(desc):
    """The bounding box of the scene's spheres and triangles (planes are unbounded)."""
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for ob in desc.objects:
        if ob[0] == "sphere":
            c, r = np.array(ob[1]), ob[2]
            lo, hi = np.minimum(lo, c - r), np.maximum(hi, c + r)
        elif ob[0] == "triangle":
            for v in ob[1:4]:
                lo, hi = np.minimum(lo, v), np.maximum(hi, v)
    return lo, hi


def incoherent_rays(name, n=NRAYS):
    """n rays with nothing in common, from a fixed-seed generator: origins uniform in the scene's bounding box, every
    tenth on or inside an object (a sphere's centre or surface point, a triangle's vertex or centroid); directions
    uniform on the sphere with lengths log-uniform in [1e-3, 1e3], every fourth turned upwards (at the sky); no zero
    components."""
    if name in _RAYS:
        return _RAYS[name]
    desc = scene(name)
    g = np.random.default_rng(20261020)
    lo, hi = scene_box(desc)
    o = g.uniform(lo, hi, (n, 3))
    objs = [ob for ob in desc.objects if ob[0] != "plane"]
    for k, i in enumerate(range(0, n, 10)):
        ob = objs[int(g.integers(len(objs)))]
        if ob[0] == "sphere":
            u = g.normal(size=3)
            o[i] = np.array(ob[1]) + (ob[2] * u / np.linalg.norm(u) if k % 2 else 0.0)
        else:
            o[i] = np.array(ob[1 + k % 3]) if k % 2 else (np.array(ob[1]) + ob[2] + ob[3]) / 3.0
    d = g.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[::4, 1] = np.abs(d[::4, 1]) + 0.5
    d *= 10.0 ** g.uniform(-3.0, 3.0, (n, 1))
    rays = np.concatenate([o, d], axis=1).astype(np.float32)
    assert not (rays[:, 3:6] == 0).any() and np.isfinite(rays).all()
    _RAYS[name] = rays
    return rays


def incoherent_oracle(name):
    """(colours, end state, summed counters) of the oracle on incoherent_rays(name) from SEED at DEPTH -- computed once."""
    if name not in _ORACLE:
        cnt = np.zeros(len(orc.COUNTER_NAMES), np.uint64)
        rgb, end = oracle_trace(scene(name), incoherent_rays(name), DEPTH, SEED, cnt)
        rgb.setflags(write=False)
        cnt.setflags(write=False)
        _ORACLE[name] = (rgb, end, cnt)
    return _ORACLE[name]
