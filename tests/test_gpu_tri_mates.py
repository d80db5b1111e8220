"""Coplanar mates on the device (rfx_intersect.h TriMates): the small-scene loops compute a mate group's z stage once per
ray.  The same scene rendered with the groups on and off (rfx_scene_set_tri_mates: off makes every triangle its own
leader, so the kernels recompute every z stage) gives the same bits, frame after frame of the random stream, with the
per-view masks built before the first frame and after a repeat; the frames with the groups on equal the CPU oracle's; the
STATS kernels' event counters do not depend on the switch."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

from reflaxman_amd import scenes
from reflaxman_amd.scenes import DIELECTRIC, METAL

pytestmark = pytest.mark.gpu

SEED = 24680
FRAMES = 3


def torture_scene():
    """A camera looking down at a floor that reaches far beyond the view, so every primary ray's line crosses a grouped
    triangle: six floor quads of mixed materials (reflections and shadows cross their seams), a raised platform of two
    overlapping coplanar triangles (equal distances: the lower object index wins) with a third triangle of its plane
    added last, a wall quad between the floor's halves in insertion order (so the floor group's members are not
    adjacent), four spheres resting on the floor (their shadow rays start on one mate and graze the others) and one
    light low over the floor."""
    s = scenes._base("mates_torture")
    s.camera = ((scenes.f32(1.0), scenes.f32(5.0), scenes.f32(0.5)), (scenes.f32(1.5), 0.0, scenes.f32(1.0)), scenes.f32(1.0))
    s.add_light((3.0, 0.8, 2.0), 0.2, (1.0, 0.95, 0.9), 0.85)
    for c, r, mt, rgb, refl in (((0.0, 0.5, 0.0), 0.5, METAL, (1.0, 1.0, 1.0), 0.9),
                                ((2.0, 0.75, 1.5), 0.75, DIELECTRIC, (0.5, 1.0, 0.3), 0.7),
                                ((1.0, 0.25, -1.0), 0.25, METAL, (1.0, 0.6, 0.4), 1.0),
                                ((-1.0, 0.4, 2.0), 0.4, DIELECTRIC, (0.2, 0.5, 1.0), 0.3)):
        s.add_sphere(c, r, mt, rgb, refl)

    def tile(i, j):
        x0, z0 = -30.0 + 20.0 * i, -20.0 + 20.0 * j
        mt = METAL if (i + j) % 2 else DIELECTRIC
        rgb = (0.4 + 0.2 * i, 0.9 - 0.3 * j, 0.5 + 0.1 * (i + j))
        s.add_triangle((x0, 0.0, z0), (x0, 0.0, z0 + 20.0), (x0 + 20.0, 0.0, z0), mt, rgb, 0.3 + 0.1 * i + 0.25 * j)
        s.add_triangle((x0, 0.0, z0 + 20.0), (x0 + 20.0, 0.0, z0 + 20.0), (x0 + 20.0, 0.0, z0), mt, rgb, 0.3 + 0.1 * i + 0.25 * j)

    for i in range(3):
        tile(i, 0)
    s.add_triangle((0.5, 0.125, -0.5), (0.5, 0.125, 1.5), (2.5, 0.125, -0.5), METAL, (1.0, 0.2, 0.2), 0.5)       # platform
    s.add_triangle((-6.0, 0.0, -6.0), (-6.0, 4.0, -6.0), (-6.0, 0.0, 8.0), METAL, (0.9, 0.9, 0.9), 0.6)          # wall
    s.add_triangle((-6.0, 4.0, -6.0), (-6.0, 4.0, 8.0), (-6.0, 0.0, 8.0), METAL, (0.9, 0.9, 0.9), 0.6)
    for i in range(3):
        tile(i, 1)
    s.add_triangle((0.5, 0.125, -0.5), (0.5, 0.125, 1.0), (2.0, 0.125, -0.5), DIELECTRIC, (0.2, 0.2, 1.0), 0.8)  # over it
    s.add_triangle((3.0, 0.125, 2.0), (3.0, 0.125, 3.0), (4.0, 0.125, 2.0), METAL, (0.9, 0.8, 0.1), 0.4)         # its plane
    return s


def scene_by_name(name):
    return torture_scene() if name == "mates_torture" else scenes.get_scene(name)


def render_frames(desc, W, H, depth, ss, masks, mates_on):
    """FRAMES consecutive frames of one renderer: [(f32 bytes, ARGB8 bytes)]."""
    from reflaxman_amd import _lib
    from reflaxman_amd.render import Renderer, build_scene, make_frame
    L = _lib.load()
    scene, cam = build_scene(desc)
    scene.set_tri_mates(mates_on)
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
    return out


@functools.lru_cache(maxsize=None)
def oracle_frames(name, W, H, depth):
    """The CPU oracle's FRAMES consecutive frames of the same random stream; computed once."""
    import oracle as orc
    o = orc.OracleRender(scene_by_name(name), SEED, 0)
    o.set_image_size(W, H)
    out = []
    for _ in range(FRAMES):
        o.render(depth, 1)
        out.append((o.image.tobytes(), o.argb().tobytes()))
    return tuple(out)


def test_the_scenes_have_groups():
    from reflaxman_amd.render import build_scene
    leader = build_scene(torture_scene())[0].tri_mates()
    floor = [t for t in range(len(leader)) if leader[t] == 0]
    assert len(floor) == 12 and max(np.diff(floor)) > 1          # the wall and the platform lie between its halves
    assert leader[6] == 6 and leader[15] == 6 and leader[16] == 6  # the platform's three, not adjacent
    assert leader[7] == 7 and leader[8] == 7                       # the wall


# masks 2: the per-view masks before the first frame; 1: from the second frame of the still view on
@pytest.mark.parametrize("masks", [2, 1])
@pytest.mark.parametrize("name,W,H,depth,ss", [("synth16", 96, 54, 8, 1), ("default", 64, 48, 4, 2),
                                               ("default", 64, 48, 4, 3), ("lights3", 96, 54, 8, 1),
                                               ("lights40", 64, 36, 8, 1), ("planes", 64, 36, 6, 1),
                                               ("mates_torture", 96, 54, 8, 1)])
def test_frames_do_not_depend_on_the_switch(name, W, H, depth, ss, masks):
    desc = scene_by_name(name)
    on = render_frames(desc, W, H, depth, ss, masks, True)
    off = render_frames(desc, W, H, depth, ss, masks, False)
    for k in range(FRAMES):
        assert on[k][0] == off[k][0], (name, masks, k, "f32")
        assert on[k][1] == off[k][1], (name, masks, k, "argb")
    assert len({f[0] for f in on}) == FRAMES  # the random stream moved on: three different frames
    if name in ("synth16", "mates_torture"):
        want = oracle_frames(name, W, H, depth)
        for k in range(FRAMES):
            assert on[k][0] == want[k][0], (name, masks, k, "f32 against the oracle")
            assert on[k][1] == want[k][1], (name, masks, k, "argb against the oracle")


def test_stats_counters_do_not_depend_on_the_switch():
    import oracle as orc
    from reflaxman_amd import _lib
    from reflaxman_amd.render import Renderer, build_scene, make_frame
    L = _lib.load()
    W, H, depth = 96, 54, 8
    got = []
    for on in (True, False):
        scene, cam = build_scene(scenes.get_scene("synth16"))
        scene.set_tri_mates(on)
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
