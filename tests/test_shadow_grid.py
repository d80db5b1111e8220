"""A far light's occluder grid (rfx_scene.cpp shadow_grid_build, rfx.h rfx_scene_shadow_grid): the host side.  No GPU.

A cell's mask must be cull_small's verdict for the bundle of every shadow ray that starts in the cell, and a point's cell
as the kernels find it (float32) must be one whose ball holds the point; then a lane's shadow ray belongs to its cell's
bundle, and the bundle cull's own bound (tests/test_bundle_cull_bound.py) says the mask keeps every object the reference
can report for it.  Checked here:
  * every cell's mask equals tests/bundle_cull.py's replay of cull_small for that cell's bundle (synth16, default, the
    far-light guard scene under the forced modes);
  * for 2^20 random points of the box and for points straddling every cell face at nextafter, the float32 cell index
    names a cell whose widened ball contains the point;
  * for 2^16 shadow rays L + rd R, half of them from points on object surfaces, every object the oracle reports as hit
    (oracle.kat, hit or any-hit flag) is in the mask of the origin's cell -- a condition: no reported hit may be dropped;
  * no grid when the light is not far, the scene is not small, there are two lights, or under mode 0;
  * the builder under ASan and UBSan through a stand-alone program (tests/native/shadow_grid_check.cpp).
"""
from __future__ import annotations

import functools
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import bundle_cull as bc
from bundle_cull import F
from reflaxman_amd import scenes
from reflaxman_amd.render import build_scene
from test_gpu_far_light import guard_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = ["synth16", "default", "far_guard"]


class Exact:
    """bundle_cull's `rng` with no perturbation: its square roots are the correctly rounded ones the host computes"""

    @staticmethod
    def uniform(lo, hi, shape):
        return np.zeros(shape)


def desc_of(name):
    return guard_scene() if name == "far_guard" else scenes.get_scene(name)


@functools.lru_cache(maxsize=None)
def grid_of(name):
    """The library's grid, records and light terms for a stock scene (the guard scene under the forced modes)."""
    scene, _ = build_scene(desc_of(name))
    if name == "far_guard":
        scene.set_far_lights(2)
        scene.set_shadow_grid(2)
    g = scene.shadow_grid()
    assert g is not None
    recs, tris, valid = scene.cull_dump()
    chosen, t = scene.far_light(0)
    assert chosen
    G = SimpleNamespace(**g, recs=recs, tris=tris, valid=valid, axis=t[1:4].copy(), near=t[5], cosa=t[6], sina=t[7])
    G.masks.setflags(write=False)
    return G


def centres(G):
    """every cell's centre as the host rounds it: corner + (i + 1/2) size in double, then float32; (nz, ny, nx, 3)"""
    nx, ny, nz = G.dims
    o, h = G.origin.astype(np.float64), float(G.cell)
    c = np.empty((nz, ny, nx, 3))
    c[..., 0] = (o[0] + (np.arange(nx) + 0.5) * h)[None, None, :]
    c[..., 1] = (o[1] + (np.arange(ny) + 0.5) * h)[None, :, None]
    c[..., 2] = (o[2] + (np.arange(nz) + 0.5) * h)[:, None, None]
    return c.astype(F)


def cell_index(G, p):
    """rfx_cull_rule.h shadow_grid_cell in float32 numpy: (inside, flat index) of points p (n, 3) float32"""
    assert p.dtype == F
    with np.errstate(invalid="ignore", over="ignore"):
        f = (p - G.origin[None, :]) * F(G.scale)
        assert f.dtype == F
        dims = np.asarray(G.dims, F)
        inside = ((f >= F(0)) & (f < dims[None, :])).all(1)
    i = np.where(inside[:, None], f, F(0)).astype(np.int32)
    nx, ny, _ = G.dims
    return inside, (i[:, 2] * ny + i[:, 1]) * nx + i[:, 0]


def pack(keep):
    return (keep.astype(np.uint64) << np.arange(64, dtype=np.uint64)[None, :]).sum(1, dtype=np.uint64)


# ------------------------------------------------------------------ geometry of the grid
@pytest.mark.parametrize("name", SCENES)
def test_box_cells_and_budget(name):
    G = grid_of(name)
    nx, ny, nz = G.dims
    assert 1 <= nx * ny * nz <= 1 << 16 and G.masks.shape == (nz, ny, nx)
    assert nx * ny * nz > 1 << 15  # the smallest cell size the budget allows, not a coarser one
    assert G.scale == F(1) / G.cell and G.cell > 0
    # the ball: the half-diagonal, widened by no more than a few percent
    hd = 0.5 * np.sqrt(3.0) * float(G.cell)
    assert hd * (1 + 1e-6 * max(G.dims)) < float(G.ball) < hd * 1.08 + 1e-6 * np.abs(G.origin).max() + 1e-30
    # the box holds every sphere's box and every triangle vertex, with room to spare
    lo = G.origin.astype(np.float64)
    hi = lo + np.asarray(G.dims) * float(G.cell)
    for ob in desc_of(name).objects:
        pts = (np.asarray(ob[1], np.float64)[None, :] + ob[2] * np.array([[-1.0] * 3, [1.0] * 3]) if ob[0] == "sphere"
               else np.asarray(ob[1:4], np.float64) if ob[0] == "triangle" else None)
        if pts is not None:
            assert (pts > lo).all() and (pts < hi).all()
    if name == "synth16":
        assert 0.3 < G.cell < 0.6  # about 0.45 units


@pytest.mark.parametrize("name", SCENES)
def test_every_mask_is_cull_smalls_verdict_for_the_cells_bundle(name):
    G = grid_of(name)
    c = centres(G).reshape(-1, 3)
    n = len(c)
    B = SimpleNamespace(c=c, a=np.broadcast_to(G.axis.astype(F), (n, 3)), rw=np.full(n, G.ball, F),
                        cosa=np.full(n, G.cosa, F), sina=np.full(n, G.sina, F), ok=np.ones(n, bool))
    keep = bc.cull_small(G.recs, G.tris, G.valid, B, Exact())
    want = pack(keep)
    got = G.masks.reshape(-1)
    assert np.array_equal(got, want), (int((got != want).sum()), n)
    # not vacuous: the masks differ from cell to cell, none holds an invalid lane, and they drop most objects
    assert len(np.unique(got)) > 20 and not (got & ~np.uint64(G.valid)).any()
    bits = np.unpackbits(got.view(np.uint8)).sum() / n
    assert bits < 0.5 * bin(G.valid).count("1"), bits
    print(f"{name}: {n} cells of {float(G.cell):.4f}, {bits:.2f} of {bin(G.valid).count('1')} objects kept per cell")


@pytest.mark.parametrize("name", SCENES)
def test_a_points_cell_holds_the_point(name):
    G = grid_of(name)
    rng = np.random.default_rng(20261101)
    lo = G.origin.astype(np.float64)
    ext = np.asarray(G.dims) * float(G.cell)
    pts = [(lo + rng.random((1 << 20, 3)) * ext).astype(F)]
    # points straddling every cell face: the face coordinate as float32, its two neighbours, the other two coordinates
    # random; the box's own outer faces among them (points just outside must fail the range test or sit in an edge cell)
    for a in range(3):
        face = (lo[a] + np.arange(G.dims[a] + 1) * float(G.cell)).astype(F)
        for v in (face, np.nextafter(face, F(-np.inf)), np.nextafter(face, F(np.inf))):
            q = (lo + rng.random((len(v) * 64, 3)) * ext).astype(F)
            q[:, a] = np.repeat(v, 64)
            pts.append(q)
    p = np.concatenate(pts)
    inside, idx = cell_index(G, p)
    assert inside[: 1 << 20].mean() > 0.999 and inside.sum() > len(p) - 64 * 6 * 3 - 2000
    c = centres(G).reshape(-1, 3).astype(np.float64)[idx[inside]]
    dist = np.linalg.norm(p[inside].astype(np.float64) - c, axis=1)
    assert dist.max() <= float(G.ball), (dist.max(), float(G.ball))
    # the ball is needed: points reach past the bare half-diagonal's 99%
    assert dist.max() > 0.99 * 0.5 * np.sqrt(3.0) * float(G.cell)
    # NaN, infinite and far points fail the range test
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e30, 0, 0], [-1e30, 1e30, 0]], F)
    assert not cell_index(G, bad)[0].any()


# ------------------------------------------------------------------ the oracle's verdicts
def surface_points(desc, n, rng):
    """n points on the scene's spheres and triangles (float32), object by object in turn"""
    objs = [ob for ob in desc.objects if ob[0] in ("sphere", "triangle")]
    out = np.empty((n, 3))
    for k in range(n):
        ob = objs[k % len(objs)]
        if ob[0] == "sphere":
            u = rng.normal(size=3)
            out[k] = np.asarray(ob[1], np.float64) + ob[2] * u / np.linalg.norm(u)
        else:
            w = rng.dirichlet([1.0, 1.0, 1.0])
            out[k] = (np.asarray(ob[1:4], np.float64) * w[:, None]).sum(0)
    return out.astype(F)


@pytest.mark.parametrize("name", ["synth16", "default"])
def test_no_reported_hit_is_dropped(name):
    import oracle as orc
    G = grid_of(name)
    desc = desc_of(name)
    rng = np.random.default_rng(20261102)
    n = 1 << 16
    lo = G.origin.astype(np.float64)
    ext = np.asarray(G.dims) * float(G.cell)
    p = np.concatenate([(lo + rng.random((n // 2, 3)) * ext).astype(F), surface_points(desc, n // 2, rng)])
    assert (np.abs(p) < G.near).all()  # inside the light's bound: dirToLight is the light's origin, bit for bit
    inside, idx = cell_index(G, p)
    assert inside.all()
    mask = G.masks.reshape(-1)[idx]
    (Lo, R, _, _), = desc.lights
    rd = rng.uniform(-1.0, 1.0, (4 * n, 3))
    rd = rd[(rd ** 2).sum(1) <= 1.0][:n].astype(F)
    rd[::4] /= np.linalg.norm(rd[::4].astype(np.float64), axis=1)[:, None].astype(F) * F(1.0000002)  # the ball's rim
    sray = np.asarray(Lo, F)[None, :] + rd * F(R)  # Scene.cpp:129 in float32
    assert sray.dtype == F and len(sray) == n
    reported = dropped = 0
    ns = nt = 0
    for ob in desc.objects:
        if ob[0] == "sphere":
            lane = (ns & 1) * 16 + (ns >> 1)
            ns += 1
            rec = np.zeros((n, 11), F)
            rec[:, 6:9], rec[:, 9] = np.asarray(ob[1], F), F(ob[2])
        elif ob[0] == "triangle":
            lane = 32 + nt
            nt += 1
            rec = np.zeros((n, 21), F)
            rec[:, 6:15] = np.asarray(ob[1:4], F).reshape(9)
        else:
            continue
        rec[:, 0:3], rec[:, 3:6] = p, sray
        res = orc.kat(ob[0], rec)
        hit = (res[:, 0] != 0) | (res[:, 14] != 0)
        reported += int(hit.sum())
        dropped += int((hit & ((mask >> np.uint64(lane)) & np.uint64(1) == 0)).sum())
    assert (G.valid >> 32) == (1 << nt) - 1 and ns + nt == bin(G.valid).count("1")
    assert dropped == 0, (dropped, reported)
    # not vacuous: the rays do meet the scene (the reference reports no hit on the sphere a ray starts on: at |ray| ~ 1e10
    # the far crossing's t rounds away, so the count is of other objects in the way)
    assert reported > n // 64
    print(f"{name}: {reported} reported hits of {n} shadow rays, none outside its cell's mask")


# ------------------------------------------------------------------ when there is no grid
def small_far_scene():
    s = scenes._base("grid")
    s.add_light((11.8e9, 4.26e9, 3.08e9), 3.48e8, (1.0, 1.0, 1.0), 0.9)
    s.add_sphere((1.0, 0.0, 0.0), 1.0, scenes.METAL, (1.0, 1.0, 1.0), 0.5)
    s.add_triangle((-2.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), scenes.METAL, (1.0, 1.0, 1.0), 0.5)
    return s


def grid_under(desc, grid=None, far=None):
    scene, _ = build_scene(desc)
    if far is not None:
        scene.set_far_lights(far)
    if grid is not None:
        scene.set_shadow_grid(grid)
    return scene.shadow_grid()


def test_the_grid_is_absent_where_it_does_not_apply():
    assert grid_under(small_far_scene()) is not None and grid_under(small_far_scene(), 2) is not None
    assert grid_under(small_far_scene(), 0) is None
    # mode 1 follows the far-light kernels; mode 2 builds for any far single light
    assert grid_under(small_far_scene(), 1, far=0) is None and grid_under(small_far_scene(), 2, far=0) is not None
    assert grid_under(guard_scene()) is None and grid_under(guard_scene(), 1, far=2) is not None
    assert grid_under(guard_scene(), 2) is not None
    near = small_far_scene()
    near.lights[0] = ((0.0, 4.26e9, 3.08e9), 3.48e8) + tuple(near.lights[0][2:])  # a zero coordinate: not far
    assert grid_under(near, 2) is None
    two = small_far_scene()
    two.add_light((1e9, 2e9, 3e9), 1e7, (1.0, 1.0, 1.0), 0.5)
    assert grid_under(two, 2) is None
    assert grid_under(scenes.get_scene("stress4096"), 2) is None  # not a small scene
    assert grid_under(scenes.get_scene("nolight"), 2) is None
    bare = scenes._base("bare")
    bare.add_light((11.8e9, 4.26e9, 3.08e9), 3.48e8, (1.0, 1.0, 1.0), 0.9)
    assert grid_under(bare, 2) is None  # nothing to bound


def test_the_setter_refuses_other_modes():
    from reflaxman_amd import _lib
    scene, _ = build_scene(small_far_scene())
    for mode in (-1, 3):
        with pytest.raises(_lib.RfxError):
            scene.set_shadow_grid(mode)


def test_a_flat_scene_keeps_the_budget():
    """one thin triangle: two of the box's edges are margins only, so the cells line up along one axis"""
    s = scenes._base("flat")
    s.add_light((11.8e9, 4.26e9, 3.08e9), 3.48e8, (1.0, 1.0, 1.0), 0.9)
    s.add_triangle((-50.0, 0.0, 0.0), (50.0, 0.0, 0.0), (0.0, 1e-3, 0.0), scenes.METAL, (1.0, 1.0, 1.0), 0.5)
    g = grid_under(s)
    assert g is not None and 1 <= np.prod(g["dims"]) <= 1 << 16 and max(g["dims"]) > 256


# ------------------------------------------------------------------ the host code under the sanitizers
def test_host_code_under_sanitizers(tmp_path):
    """rfx_scene.cpp with a stand-alone checker (tests/native/shadow_grid_check.cpp) by plain g++ under ASan and UBSan:
    no HIP, nothing loaded into Python."""
    csrc = os.path.join(ROOT, "reflaxman_amd", "csrc")
    exe = str(tmp_path / "shadow_grid_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + csrc, os.path.join(csrc, "rfx_scene.cpp"),
                    os.path.join(ROOT, "tests", "native", "shadow_grid_check.cpp"), "-o", exe, "-lm"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == ""
