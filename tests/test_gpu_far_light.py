"""Far lights on the device (rfx_bounce.h FARL, rfx_bundle.h make_bundle_far): a small scene whose one light is far reads
the light's constant terms and the shadow rays' cone from the light's record at every hit inside the light's bound.  The
same scene with the switch off (rfx_scene_set_far_lights 0: the general kernels) gives the same bits, frame after frame
of the random stream, with and without the per-view masks; the frames with it on equal the CPU oracle's; a scene whose
hits lie on both sides of its light's bound does too; the far and the general form of every term agree bit for bit at
2^20 points; the STATS kernels' event counters do not depend on the switch."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

from reflaxman_amd import scenes
from reflaxman_amd.scenes import DIELECTRIC, METAL

pytestmark = pytest.mark.gpu

SEED = 13579
FRAMES = 3
GUARD_LIGHT = ((9.0e6, 1.1e7, 1.2e7), 3.0e5)  # floats 1 apart just below each coordinate: the bound is 0.5


def guard_scene():
    """Eight spheres and a ground quad spanning +-3 under one far light whose bound is 0.5: the hits of one wave lie on
    both sides of it, so its lanes split between the record's terms and the general expressions, and its shadow
    bundles between the record's cone and the one found from the rays."""
    s = scenes._base("far_guard")
    s.camera = ((0.0, scenes.f32(2.5), scenes.f32(-7.0)), (0.0, scenes.f32(0.3), 0.0), scenes.f32(1.0))
    s.add_light(*GUARD_LIGHT, (1.0, 0.97, 0.9), 0.9)
    for k, (x, z) in enumerate(((-0.3, -0.3), (0.35, 0.2), (-0.1, 0.6), (1.2, -0.4), (-1.4, 0.5), (2.3, 1.5), (-2.4, -1.2),
                                (0.6, -1.6))):
        r = 0.25 + 0.05 * (k % 3)
        s.add_sphere((x, r, z), r, DIELECTRIC if k % 2 else METAL, (0.4 + 0.07 * k, 1.0 - 0.08 * k, 0.5 + 0.05 * (k % 4)),
                     0.2 + 0.1 * k)
    s.add_triangle((-3.0, 0.0, -3.0), (-3.0, 0.0, 3.0), (3.0, 0.0, -3.0), METAL, (0.8, 0.8, 0.7), 0.5)
    s.add_triangle((-3.0, 0.0, 3.0), (3.0, 0.0, 3.0), (3.0, 0.0, -3.0), DIELECTRIC, (0.6, 0.8, 0.9), 0.6)
    return s


def scene_by_name(name):
    return guard_scene() if name == "far_guard" else scenes.get_scene(name)


def render_frames(desc, W, H, depth, ss, masks, mode):
    """FRAMES consecutive frames of one renderer: (whether the far-light kernels were chosen, [(f32, ARGB8) bytes])."""
    from reflaxman_amd import _lib
    from reflaxman_amd.render import Renderer, build_scene, make_frame
    L = _lib.load()
    scene, cam = build_scene(desc)
    scene.set_far_lights(mode)
    chosen = scene.far_light(0)[0]
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
    return chosen, out


@functools.lru_cache(maxsize=None)
def oracle_frames(name, W, H, depth, ss):
    """The CPU oracle's FRAMES consecutive frames of the same random stream; computed once per case."""
    import oracle as orc
    o = orc.OracleRender(scene_by_name(name), SEED, 0)
    o.set_image_size(W, H)
    out = []
    for _ in range(FRAMES):
        o.render(depth, ss)
        out.append((o.image.tobytes(), o.argb().tobytes()))
    return tuple(out)


def assert_same_frames(a, b, what):
    for k in range(FRAMES):
        assert a[k][0] == b[k][0], (*what, k, "f32")
        assert a[k][1] == b[k][1], (*what, k, "argb")


# masks 2: the per-view masks before every launch; 0: none, so the first segment's shadow bundles take the cone too
@pytest.mark.parametrize("masks", [2, 0])
@pytest.mark.parametrize("name,W,H,depth,ss", [("synth16", 160, 90, 8, 1), ("default", 160, 120, 4, 1),
                                               ("default", 96, 64, 4, 2), ("default", 7, 3, 8, 1)])
def test_frames_do_not_depend_on_the_switch(name, W, H, depth, ss, masks):
    desc = scene_by_name(name)
    chosen, on = render_frames(desc, W, H, depth, ss, masks, 1)
    off_chosen, off = render_frames(desc, W, H, depth, ss, masks, 0)
    assert chosen and not off_chosen  # the stock scenes' sun is far and they fit its bound
    assert_same_frames(on, off, (name, masks, "modes 1 and 0"))
    assert len({f[0] for f in on}) == FRAMES  # the random stream moved on: three different frames
    assert_same_frames(on, oracle_frames(name, W, H, depth, ss), (name, masks, "mode 1 against the oracle"))


@pytest.mark.parametrize("masks", [2, 0])
def test_hits_on_both_sides_of_the_bound(masks):
    from reflaxman_amd.render import build_scene
    desc = guard_scene()
    scene = build_scene(desc)[0]
    assert not scene.far_light(0)[0] and scene.far_light(0)[1][5] == 0.5  # far, but the scene is wider than the bound
    W, H, depth = 160, 90, 8
    chosen, forced = render_frames(desc, W, H, depth, 1, masks, 2)
    off_chosen, off = render_frames(desc, W, H, depth, 1, masks, 0)
    assert chosen and not off_chosen
    assert_same_frames(forced, off, ("far_guard", masks, "modes 2 and 0"))
    assert_same_frames(forced, oracle_frames("far_guard", W, H, depth, 1), ("far_guard", masks, "mode 2 against the oracle"))
    lit = np.frombuffer(forced[0][0], np.float32).reshape(H, W, 3)
    assert lit.max() > 0.5 and len(np.unique(lit.round(2))) > 20  # a lit, shaded picture, not a flat one


def test_a_far_eye_and_a_ray_batch_from_far_away():
    """Hits of rays that start 1e5 away carry a float error far above their distance to anything: a frame from such an
    eye and a caller's batch of such rays give the same bits with the switch on and off."""
    from reflaxman_amd.render import Renderer, build_scene
    desc = scenes.get_scene("synth16")
    eye, at, _ = desc.camera
    d = np.asarray(eye, np.float64) - np.asarray(at, np.float64)
    far_eye = np.asarray(at, np.float64) + d / np.linalg.norm(d) * 1.0e5
    desc.camera = (tuple(scenes.f32(v) for v in far_eye), at, scenes.f32(1.0e-4))
    chosen, on = render_frames(desc, 96, 54, 8, 1, 2, 1)
    _, off = render_frames(desc, 96, 54, 8, 1, 2, 0)
    assert chosen
    assert_same_frames(on, off, ("synth16 from 1e5 away", "modes 1 and 0"))
    assert len(set(np.frombuffer(on[0][1], np.uint32).tolist())) > 8  # the scene is in view
    rng = np.random.default_rng(5)
    n = 4096
    target = np.asarray(at, np.float64) + rng.uniform(-3.0, 3.0, (n, 3))
    origin = target + (d / np.linalg.norm(d) + rng.uniform(-0.2, 0.2, (n, 3))) * 1.0e5
    rays = np.concatenate([origin, target - origin], axis=1).astype(np.float32)
    got = []
    for mode in (1, 0):
        scene, _ = build_scene(scenes.get_scene("synth16"))
        scene.set_far_lights(mode)
        r = Renderer(sphere_seed=SEED, jitter_seed=0)
        r.set_scene(scene)
        got.append(r.trace_rays(rays, 8).tobytes())
        r.close()
    assert got[0] == got[1]


@pytest.mark.parametrize("name,n", [("synth16", 1 << 20), ("far_guard", 1 << 18)])
def test_far_and_general_forms_agree_bit_for_bit(name, n):
    from reflaxman_amd.render import Renderer, build_scene
    scene, _ = build_scene(scene_by_name(name))
    scene.set_far_lights(2)
    chosen, t = scene.far_light(0)
    near = t[5]
    assert chosen and near > 0
    L = np.asarray(scene_by_name(name).lights[0][0], np.float32)
    rng = np.random.default_rng(99)
    pts = rng.uniform(-2.0 * float(near), 2.0 * float(near), (n, 3)).astype(np.float32)
    third = n // 3
    pts[:third] *= np.float32(0.5)  # a third wholly inside the bound; the rest straddle it coordinate by coordinate
    inner = np.nextafter(near, np.float32(0))
    outer = np.nextafter(near, np.float32(np.inf))
    edge = np.array([inner, -inner, near, -near, outer, -outer, 0.0, -0.0], np.float32)
    pts[-512:] = edge[rng.integers(0, len(edge), (512, 3))]
    r = Renderer(sphere_seed=SEED)
    r.set_scene(scene)
    out = r.kat_far_light(pts)
    r.close()
    assert not np.isnan(out).any()  # the kernel writes NaN where the far form differs from the general one
    inside = (np.abs(pts) < near).all(axis=1)
    assert n // 4 < inside.sum() < n // 2 and (~inside[-512:]).any() and inside[-512:].any()
    record = np.concatenate([L, t[:5]]).astype(np.float32)
    assert np.array_equal(out[inside].view(np.uint32), np.broadcast_to(record.view(np.uint32), out[inside].shape))
    want = L[None, :] - pts[~inside]  # outside: the general form's difference, in float32
    assert np.array_equal(out[~inside, :3].view(np.uint32), want.view(np.uint32))
    assert (out[~inside, :3] != L[None, :]).any()


def test_stats_counters_do_not_depend_on_the_switch():
    import oracle as orc
    from reflaxman_amd import _lib
    from reflaxman_amd.render import Renderer, build_scene, make_frame
    L = _lib.load()
    W, H, depth = 96, 54, 8
    got = []
    for mode in (1, 0):
        scene, cam = build_scene(scenes.get_scene("synth16"))
        scene.set_far_lights(mode)
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
