"""Triangle BVH of non-small scenes (rfx_renderer_set_tri_accel): every frame equals the reference's, byte for byte,
with the tree (mode 1; mode 2: narrow bundles walk it too) and without it (mode 0), in every kernel that traces a non-small scene -- the plain trace, the
park and both bounce kernels, the SSAA lane and per-pixel forms, block preview -- and the stats kernel's event counters
stay the oracle's.  The oracle is the CPU restatement (oracle/), itself checked against the reference's hashes of the
degenerate scene (tests/golden/tri_accel, tests/test_tri_accel_golden.py).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from helpers import GOLDEN, sha
from reflaxman_amd import _lib, scenes

pytestmark = pytest.mark.gpu
SEED = 1350490027

_DESC, _REF = {}, {}


def desc_of(key):
    """key: ('mesh', nx, nz) | ('soup', n, n_spheres) | ('degenerate',) | ('default',)"""
    if key not in _DESC:
        _DESC[key] = (scenes.mesh_scene(*key[1:]) if key[0] == "mesh" else
                      scenes.soup_scene(key[1], n_spheres=key[2]) if key[0] == "soup" else
                      scenes.degenerate_soup_scene() if key[0] == "degenerate" else scenes.default_scene())
    return _DESC[key]


_BUILT = {}


def built(key):
    """(Scene, Camera) of a case, built once: a Scene serves any number of renderers"""
    if key not in _BUILT:
        from reflaxman_amd.render import build_scene
        _BUILT[key] = build_scene(desc_of(key))
    return _BUILT[key]


def reference(key, W, H, depth, ss=1, additive=False, frames=1):
    """The oracle's stored float frame after `frames` frames (computed once per case, shared, read-only)."""
    k = (key, W, H, depth, ss, additive, frames)
    if k not in _REF:
        import oracle as orc
        o = orc.OracleRender(desc_of(key), SEED, 0)
        o.set_image_size(W, H)
        for _ in range(frames):
            o.render(depth, ss, additive)
        o.image.setflags(write=False)
        _REF[k] = o.image
    return _REF[k]


def render(key, W, H, depth, mode, ss=1, additive=False, frames=1, chunks=None, **knobs):
    """The stored float frame through the Python mirror of Render under tri-accel `mode`; returns (image, renderer
    facts).  knobs: Renderer.set_<name>(value) calls."""
    from reflaxman_amd.render import Render
    r = Render(sphere_seed=SEED, jitter_seed=0, load_default_scene=False)
    r.scene, r.camera = built(key)
    r.setImageSize(W, H)
    r._r.set_tri_accel(mode)
    for name, v in knobs.items():
        getattr(r._r, "set_" + name)(v)
    for _ in range(frames):
        r.renderBegin(depth, ss, additive)
        i = 0
        while r.renderNext(W * H if chunks is None else chunks[i % len(chunks)]):
            i += 1
    r.synchronize()
    img = r.image.copy()
    info = r._r.accel_info()
    facts = {"tri_nodes": info.tri_nodes, "sph_nodes": info.sph_nodes, "bounce_form": r._r.bounce_form(),
             "leaf": info.tri_leaf_size, "in_leaves": info.tri_in_leaves, "residual": info.tri_residual,
             "depth": info.tri_depth, "narrow": info.narrow_tri_bvh}
    r.close()
    return img, facts


def both_modes(key, W, H, depth, expect_tree=True, **kw):
    ref = reference(key, W, H, depth, kw.get("ss", 1), kw.get("additive", False), kw.get("frames", 1))
    out = {}
    for mode in (0, 1, 2):
        img, facts = render(key, W, H, depth, mode, **kw)
        assert img.tobytes() == ref.tobytes(), (key, mode, kw, int((img != ref).any(axis=2).sum()))
        if mode == 0:
            assert facts["tri_nodes"] == 0
        elif expect_tree:
            assert facts["tri_nodes"] > 0 and 0 < facts["depth"] <= 16 and facts["narrow"] == (mode == 2)
        out[mode] = facts
    return out


MESH = ("mesh", 16, 12)


@pytest.mark.parametrize("kw", [{}, {"regroup": 0}, {"regroup": 1}, {"tile_order": 3}, {"chunks": [100, 37]},
                                {"launch_traces": 500}], ids=str)
def test_mesh_plain_frames(kw):
    """384 triangles under 8 spheres (no sphere BVH): trace + park + the global bounce kernel, the unparked trace,
    the sorted schedule, renderNext spans, split launches."""
    f = both_modes(MESH, 64, 36, 6, **kw)
    assert f[1]["sph_nodes"] == 0 and f[1]["in_leaves"] + f[1]["residual"] == 384


@pytest.mark.parametrize("W,H,kw", [(32, 18, {"ss": 2, "additive": True, "frames": 2}), (32, 18, {"ss": 4}),
                                    (16, 9, {"ss": 16}), (48, 27, {"ss": -3})], ids=str)
def test_mesh_ssaa_and_block_preview(W, H, kw):
    """the SSAA lane forms (2 x 2 jittered and accumulated over two frames, 4 x 4), the wave-per-pixel form
    (16 x 16) and the block preview"""
    both_modes(MESH, W, H, 6, **kw)


def test_soup_with_spheres_both_trees():
    """1500 soup triangles and 300 spheres: the sphere BVH and the triangle BVH in one walk order, in the parked
    frame's LDS-staged bounce kernel (sphere nodes in LDS, triangle nodes in global memory) and the global form"""
    key = ("soup", 1500, 300)
    f = both_modes(key, 48, 27, 6)
    assert f[1]["sph_nodes"] > 0 and f[1]["bounce_form"] == f[0]["bounce_form"] == 2
    f = both_modes(key, 48, 27, 6, regroup=0)
    assert f[1]["bounce_form"] == 0


@pytest.mark.parametrize("n", [33, 65, 127, 129])
def test_soup_leaf_edges(n):
    """triangle counts around the 64-wide chunks of mode 0 and with a partly filled last leaf in mode 1"""
    f = both_modes(("soup", n, 0), 24, 14, 4)
    assert f[1]["in_leaves"] + f[1]["residual"] == n + 2


def test_degenerate_scene_against_reference_hash():
    """slivers, zero-area triangles (residual list) and coincident pairs (the tie rule): the reference's own frame"""
    g = json.load(open(os.path.join(GOLDEN, "tri_accel", "soup300_degenerate_48x27_d8.json")))
    for mode in (0, 1, 2):
        img, facts = render(("degenerate",), g["W"], g["H"], g["depth"], mode)
        assert sha(img) == g["sha_f32"], mode
        if mode:
            assert facts["tri_nodes"] > 0 and facts["residual"] >= 14


def test_large_mesh_with_or_without_tree():
    """132,000 triangles: more leaves than the kernels' int16 stack slots name -- bit-exact whether or not a tree
    was built"""
    both_modes(("mesh", 300, 220), 16, 9, 2, expect_tree=False)


def test_event_counters_under_mode_1():
    """the stats kernel keeps the reference's loops whatever the mode: its counters equal the oracle's"""
    import oracle as orc
    from reflaxman_amd.render import Renderer, make_frame
    desc = desc_of(MESH)
    W, H, depth = 48, 27, 6
    o = orc.OracleRender(desc, 4242, 0)
    o.set_image_size(W, H)
    oc = np.zeros(len(orc.COUNTER_NAMES), np.uint64)
    o.render(depth, 1, counters=oc)
    s, cam = built(MESH)
    rr = Renderer(sphere_seed=4242)
    rr.set_tri_accel(1)
    rr.set_scene(s)
    assert rr.accel_info().tri_nodes > 0
    img = np.zeros((H, W, 3), np.float32)
    gc = np.zeros(len(orc.COUNTER_NAMES), np.uint64)
    f = make_frame(cam, W, H, depth, 1)
    _lib.check(_lib.load().rfx_render_frame_host(rr._h, C.byref(f), _lib.fptr(img), None, _lib.u64ptr(gc)))
    assert img.tobytes() == o.image.tobytes()
    skip = {k for k in orc.COUNTER_NAMES if k.startswith("sh_")} if desc.n_spheres > 32 else set()
    bad = {k: (int(a), int(b)) for k, a, b in zip(orc.COUNTER_NAMES, gc, oc) if a != b and k not in skip}
    assert not bad, bad
    rr.close()


def test_scene_changes_on_one_renderer():
    """mesh, the default small scene, the mesh again on one renderer: every frame the reference's, the tree gone and
    back"""
    from reflaxman_amd.render import Render
    W, H, depth = 64, 36, 6
    r = Render(sphere_seed=SEED, jitter_seed=0, load_default_scene=False)
    r.setImageSize(W, H)
    r._r.set_tri_accel(1)
    import oracle as orc
    for k in (MESH, ("default",), MESH):
        r.scene, r.camera = built(k)
        seed = r.getRng()[0]
        r.renderBegin(depth, 1, False)
        while r.renderNext(W * H):
            pass
        r.synchronize()
        o = orc.OracleRender(desc_of(k), seed, 0)
        o.set_image_size(W, H)
        o.render(depth, 1)
        assert r.image.tobytes() == o.image.tobytes(), k
        assert (r._r.accel_info().tri_nodes > 0) == (k == MESH)
    r.close()


def test_two_member_group_renders_the_soup():
    """a device group of two members on one device, each with its own tree: the single renderer's frame"""
    import torch
    from reflaxman_amd.render import Renderer, make_frame
    L = _lib.load()
    scene, cam = built(("soup", 1500, 300))
    W, H = 48, 32
    g = C.c_void_p()
    _lib.check(L.rfx_group_create(C.byref(g), (C.c_int * 2)(0, 0), 2), "group_create")
    for m in range(2):
        _lib.check(L.rfx_renderer_set_tri_accel(C.c_void_p(L.rfx_group_renderer(g, m)), 1))
    _lib.check(L.rfx_group_set_scene(g, scene._h), "group_set_scene")
    info = _lib.AccelInfo()
    for m in range(2):
        _lib.check(L.rfx_renderer_accel_info(C.c_void_p(L.rfx_group_renderer(g, m)), C.byref(info)))
        assert info.tri_nodes > 0 and info.sph_nodes > 0
    _lib.check(L.rfx_renderer_set_rng(C.c_void_p(L.rfx_group_renderer(g, 0)), SEED, 7))
    one = Renderer(sphere_seed=SEED, jitter_seed=7)
    one.set_tri_accel(0)
    one.set_scene(scene)
    f = make_frame(cam, W, H, 6, 1)
    bufs = [torch.zeros(H * W * 3, dtype=torch.float32, device="cuda") for _ in range(2)]
    argb = [torch.zeros(H * W, dtype=torch.int32, device="cuda") for _ in range(2)]
    _lib.check(L.rfx_group_render_frame(g, C.byref(f), C.c_void_p(bufs[0].data_ptr()), C.c_void_p(argb[0].data_ptr()), None))
    one.render_frame(f, bufs[1].data_ptr(), argb[1].data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(bufs[0], bufs[1]) and torch.equal(argb[0], argb[1])
    ref = reference(("soup", 1500, 300), W, H, 6)
    assert bufs[0].cpu().numpy().tobytes() == ref.tobytes()
    L.rfx_group_destroy(g)
    one.close()
