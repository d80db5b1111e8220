"""A far light's occluder grid on the device (rfx_bounce.h GRID): a wave of the far-light kernels whose facing hits all
lie inside the light's bound and the grid's box takes its shadow mask from its lanes' cells instead of culling its own
bundle.  The grid only ever skips tests that miss, so the same scene without it (rfx_scene_set_shadow_grid 0) gives the
same bits, frame after frame of the random stream, with and without the per-view masks, and both equal the CPU oracle's
frames; a scene whose hits lie on both sides of the light's bound, a scene with planes (hits outside the box) and a
frame from an eye 1e5 away fall back wave by wave and still match; the STATS kernels' event counters do not depend on
the switch."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from reflaxman_amd import scenes
from test_gpu_far_light import FRAMES, SEED, assert_same_frames, guard_scene, oracle_frames, scene_by_name

pytestmark = pytest.mark.gpu


def render_frames(desc, W, H, depth, ss, masks, grid, far=None):
    """FRAMES consecutive frames of one renderer: (cells of the grid the scene uploads, [(f32, ARGB8) bytes])."""
    from reflaxman_amd import _lib
    from reflaxman_amd.render import Renderer, build_scene, make_frame
    L = _lib.load()
    scene, cam = build_scene(desc)
    if far is not None:
        scene.set_far_lights(far)
    scene.set_shadow_grid(grid)
    g = scene.shadow_grid()
    assert scene.far_light(0)[0]  # every case here runs the far-light kernels
    r = Renderer(sphere_seed=SEED, jitter_seed=0)
    r.set_scene(scene)
    r.set_prim_masks(masks)
    d_img, d_argb = C.c_void_p(), C.c_void_p()
    _lib.check(L.rfx_device_alloc(r._h, W * H * 12, C.byref(d_img)))
    _lib.check(L.rfx_device_alloc(r._h, W * H * 4, C.byref(d_argb)))
    out = []
    f = make_frame(cam, W, H, depth, ss)
    for _ in range(FRAMES):
        r.render_frame(f, d_img.value, d_argb.value)
        r.synchronize()
        rgb, argb = np.empty(W * H * 3, np.float32), np.empty(W * H, np.uint32)
        _lib.check(L.rfx_memcpy_d2h(r._h, rgb.ctypes.data_as(C.c_void_p), d_img, rgb.nbytes))
        _lib.check(L.rfx_memcpy_d2h(r._h, argb.ctypes.data_as(C.c_void_p), d_argb, argb.nbytes))
        out.append((rgb.tobytes(), argb.tobytes()))
    L.rfx_device_free(r._h, d_img)
    L.rfx_device_free(r._h, d_argb)
    r.close()
    return (0 if g is None else int(np.prod(g["dims"]))), out


# masks 2: the per-view masks before every launch; 0: none, so the first segment's shadow bundles take the grid too
@pytest.mark.parametrize("masks", [2, 0])
@pytest.mark.parametrize("name,W,H,depth,ss", [("synth16", 160, 90, 8, 1), ("default", 160, 120, 4, 1),
                                               ("default", 96, 64, 4, 2), ("default", 7, 3, 8, 1)])
def test_frames_do_not_depend_on_the_grid(name, W, H, depth, ss, masks):
    desc = scene_by_name(name)
    cells, on = render_frames(desc, W, H, depth, ss, masks, 1)
    off_cells, off = render_frames(desc, W, H, depth, ss, masks, 0)
    assert cells > 1 << 15 and off_cells == 0  # the stock scenes get the grid by default
    assert_same_frames(on, off, (name, masks, "modes 1 and 0"))
    assert len({f[0] for f in on}) == FRAMES  # the random stream moved on: three different frames
    assert_same_frames(on, oracle_frames(name, W, H, depth, ss), (name, masks, "mode 1 against the oracle"))


@pytest.mark.parametrize("masks", [2, 0])
def test_hits_on_both_sides_of_the_lights_bound(masks):
    """The far-light tests' guard scene: its light's bound is 0.5 and its objects span +-3, so the cells are coarse
    against the bound and most waves hold a facing hit outside it: those take the bundle path, the others the grid."""
    desc = guard_scene()
    W, H, depth = 160, 90, 8
    cells, forced = render_frames(desc, W, H, depth, 1, masks, 2, far=2)
    off_cells, off = render_frames(desc, W, H, depth, 1, masks, 0, far=2)
    assert cells > 1 << 15 and off_cells == 0
    assert_same_frames(forced, off, ("far_guard", masks, "modes 2 and 0"))
    assert_same_frames(forced, oracle_frames("far_guard", W, H, depth, 1), ("far_guard", masks, "mode 2 against the oracle"))


@pytest.mark.parametrize("masks", [2, 0])
def test_planes_put_hits_outside_the_box(masks):
    """cfg 173: the planes reach past the box of the spheres and triangles, so waves fall back hit by hit"""
    desc = scenes.get_scene("planes")
    W, H, depth = 160, 90, 8
    cells, on = render_frames(desc, W, H, depth, 1, masks, 1)
    _, off = render_frames(desc, W, H, depth, 1, masks, 0)
    assert cells > 1 << 15
    assert_same_frames(on, off, ("planes", masks, "modes 1 and 0"))
    assert_same_frames(on, oracle_frames("planes", W, H, depth, 1), ("planes", masks, "mode 1 against the oracle"))


def test_a_far_eye():
    """Hits of rays that start 1e5 away carry a float error far above a cell: wherever they land, inside the box or
    not, the frame has the same bits with the grid and without."""
    desc = scenes.get_scene("synth16")
    eye, at, _ = desc.camera
    d = np.asarray(eye, np.float64) - np.asarray(at, np.float64)
    far_eye = np.asarray(at, np.float64) + d / np.linalg.norm(d) * 1.0e5
    desc.camera = (tuple(scenes.f32(v) for v in far_eye), at, scenes.f32(1.0e-4))
    cells, on = render_frames(desc, 96, 54, 8, 1, 2, 1)
    _, off = render_frames(desc, 96, 54, 8, 1, 2, 0)
    assert cells > 1 << 15
    assert_same_frames(on, off, ("synth16 from 1e5 away", "modes 1 and 0"))
    assert len(set(np.frombuffer(on[0][1], np.uint32).tolist())) > 8  # the scene is in view


def test_stats_counters_do_not_depend_on_the_grid():
    import oracle as orc
    from reflaxman_amd import _lib
    from reflaxman_amd.render import Renderer, build_scene, make_frame
    L = _lib.load()
    W, H, depth = 96, 54, 8
    got = []
    for mode in (1, 0):
        scene, cam = build_scene(scenes.get_scene("synth16"))
        scene.set_shadow_grid(mode)
        r = Renderer(sphere_seed=SEED)
        r.set_scene(scene)
        img = np.zeros((H, W, 3), np.float32)
        cnt = np.zeros(len(orc.COUNTER_NAMES), np.uint64)
        f = make_frame(cam, W, H, depth, 1)
        _lib.check(L.rfx_render_frame_host(r._h, C.byref(f), _lib.fptr(img), None, _lib.u64ptr(cnt)))
        got.append((img.tobytes(), cnt.copy()))
        r.close()
    assert got[0][0] == got[1][0]
    assert np.array_equal(got[0][1], got[1][1]) and got[0][1].sum() > 0
