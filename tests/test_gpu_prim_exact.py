"""The per-view masks narrowed to the view's known primary hits (rfx_renderer_set_prim_exact, prim_cull_kernel):
word 0 of a tile is the set of its winners, and a shadow word drops the one object all the tile's lit hits lie on.
The narrowed words are subsets of the conservative ones, match a float64 replay of the primary rays, and change no
pixel on any path that builds masks."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

from reflaxman_amd import scenes

pytestmark = pytest.mark.gpu

STRIDE = 5  # words per wave tile: the closest-hit mask, then one shadow mask per light up to 4 (rfx.h)
SEED = 97531


class Rig:
    """One renderer, one scene and caller-owned frame buffers: frames through rfx_render_frame (or, for a strip of a
    multi-rank frame, the counted entry point with every rank's slice counted here)."""

    def __init__(self, desc, W, H, masks, exact=None, jitter_seed=99):
        from reflaxman_amd import _lib
        from reflaxman_amd.render import Renderer, build_scene
        self.L = _lib.load()
        self.check = _lib.check
        self.scene, self.cam = build_scene(desc)
        self.W, self.H = W, H
        self.r = Renderer(sphere_seed=SEED, jitter_seed=jitter_seed)
        self.r.set_scene(self.scene)
        self.r.set_prim_masks(masks)
        if exact is not None:
            self.r.set_prim_exact(exact)
        self.d_img, self.d_argb, self.d_cnt = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self.check(self.L.rfx_device_alloc(self.r._h, W * H * 12, C.byref(self.d_img)))
        self.check(self.L.rfx_device_alloc(self.r._h, W * H * 4, C.byref(self.d_argb)))
        zero = np.zeros(W * H * 3, np.float32)  # a sub-range or a strip leaves the rest of the buffers as they are
        self.check(self.L.rfx_memcpy_h2d(self.r._h, self.d_img, zero.ctypes.data_as(C.c_void_p), W * H * 12))
        self.check(self.L.rfx_memcpy_h2d(self.r._h, self.d_argb, zero.ctypes.data_as(C.c_void_p), W * H * 4))

    def frame(self, depth, ss=1, additive=False, **kw):
        """Render one frame; returns its (f32 bytes, ARGB8 bytes)."""
        from reflaxman_amd.render import make_frame
        f = make_frame(self.cam, self.W, self.H, depth, ss, additive=additive, **kw)
        if f.nranks > 1:
            n = f.nranks
            bps = C.c_uint64()
            self.check(self.L.rfx_frame_rng_blocks(self.r._h, C.byref(f), n, C.byref(bps)))
            if not self.d_cnt:
                self.check(self.L.rfx_device_alloc(self.r._h, n * bps.value * 4, C.byref(self.d_cnt)))
            for sl in range(n):  # what the all-gather assembles from every rank's slice
                self.check(self.L.rfx_frame_rng_count(self.r._h, C.byref(f), sl, n, self.d_cnt, None))
            self.check(self.L.rfx_render_frame_counted(self.r._h, C.byref(f), n, self.d_cnt, self.d_img, self.d_argb,
                                                       None, None))
        else:
            self.r.render_frame(f, self.d_img.value, self.d_argb.value)
        self.r.synchronize()
        rgb = np.empty(self.W * self.H * 3, np.float32)
        argb = np.empty(self.W * self.H, np.uint32)
        self.check(self.L.rfx_memcpy_d2h(self.r._h, rgb.ctypes.data_as(C.c_void_p), self.d_img, rgb.nbytes))
        self.check(self.L.rfx_memcpy_d2h(self.r._h, argb.ctypes.data_as(C.c_void_p), self.d_argb, argb.nbytes))
        return rgb.tobytes(), argb.tobytes()

    def masks(self, rows=None):
        """The masks held, as (tile rows, tiles per row, STRIDE); rows: pixel rows of the launch (default H)."""
        m = self.r.prim_masks()
        ty = -(-(self.H if rows is None else rows) // 8)
        assert m.size and m.size % (STRIDE * ty) == 0, (m.size, ty)
        return m.reshape(ty, -1, STRIDE)

    def close(self):
        for d in (self.d_img, self.d_argb, self.d_cnt):
            if d:
                self.L.rfx_device_free(self.r._h, d)
        self.r.close()


def popcount(a) -> int:
    return int(np.unpackbits(np.ascontiguousarray(a).view(np.uint8)).sum())


@functools.lru_cache(maxsize=None)
def both_masks(name, W, H, depth):
    """(conservative, exact) read-backs of one still view, masks built before every launch; computed once."""
    out = []
    for exact in (0, 1):
        g = Rig(scenes.get_scene(name), W, H, 2, exact)
        g.frame(depth)
        m = g.masks().copy()
        m.setflags(write=False)
        out.append(m)
        g.close()
    return tuple(out)


# ------------------------------------------------------------------ the float64 replay of the primary rays
def sphere_bit(i):
    return (i & 1) * 16 + (i >> 1)


def winners(desc, o, ray):
    """Per ray (float64): the winner's mask bit (-1: nothing hit) and whether the call is too close -- a runner-up
    within 1e-4 relative of the winner's distance, or a triangle winner within 1e-4 of an edge in u, v or u + v.
    Sphere.cpp:44-85 (the nearer root, positive), Triangle.cpp:53-108 (two-sided, u, v >= 0, u + v < 1)."""
    dist, bits, edge = [], [], []
    raylen = np.linalg.norm(ray, axis=-1)
    ns = nt = 0
    for ob in desc.objects:
        if ob[0] == "sphere":
            c, r = np.array(ob[1], np.float64), float(ob[2])
            vco = o - c
            a = (ray * ray).sum(-1)
            b = 2.0 * (ray @ vco)
            d = b * b - 4.0 * a * (vco @ vco - r * r)
            with np.errstate(invalid="ignore"):
                t = (-b - np.sqrt(d)) / (2.0 * a)
            ok = (d >= 0) & (t > 0)
            dist.append(np.where(ok, t * raylen, np.inf))
            bits.append(sphere_bit(ns))
            edge.append(np.zeros(raylen.shape, bool))
            ns += 1
        elif ob[0] == "triangle":
            v0, v1, v2 = (np.array(v, np.float64) for v in ob[1:4])
            A, B = v2 - v0, v1 - v0
            inv = np.linalg.inv(np.stack([A, B, np.cross(A, B)], 1))  # o + t ray = v0 + u A + v B
            ao, ar = inv @ (o - v0), ray @ inv.T
            with np.errstate(divide="ignore", invalid="ignore"):
                t = -ao[2] / ar[..., 2]
                u, v = ao[0] + t * ar[..., 0], ao[1] + t * ar[..., 1]
                ok = (t > 0) & (u >= 0) & (v >= 0) & (u + v < 1)
                near = (np.abs(u) < 1e-4) | (np.abs(v) < 1e-4) | (np.abs(u + v - 1) < 1e-4)
            dist.append(np.where(ok, t * raylen, np.inf))
            bits.append(32 + nt)
            edge.append(near & ok)
            nt += 1
        else:
            raise AssertionError("the replay knows spheres and triangles only")
    dist = np.stack(dist)
    order = np.argsort(dist, axis=0, kind="stable")
    d1 = np.take_along_axis(dist, order[:1], 0)[0]
    d2 = np.take_along_axis(dist, order[1:2], 0)[0]
    hit = np.isfinite(d1)
    win = np.where(hit, np.array(bits)[order[0]], -1)
    with np.errstate(invalid="ignore"):
        close = hit & np.isfinite(d2) & (d2 - d1 < 1e-4 * d1)
    close |= np.take_along_axis(np.stack(edge), order[:1], 0)[0] & hit
    return win, close


PROBE = 1.0 / 16  # pixels


@functools.lru_cache(maxsize=None)
def replay(name, W, H):
    """Each pixel's primary winner recomputed in float64 from the SceneDesc, as its mask bit (-1: nothing hit), and the
    pixels to ignore: a winner too close to call (winners), or another winner next to the pixel.

    "Next to" is taken at PROBE = 1/16 pixel -- the eight rays offset by that much in x and y around the pixel's own --
    not at the neighbouring pixels: at these frame sizes the 8 neighbours alone rule out 26.4% of 64x40 (4 neighbours:
    20.4%) and 12.7% of 160x90, over the 10% cap before the renderer has been asked anything; the probes rule out the
    same silhouettes where they pass within 1/16 pixel of the ray, some 10^4 times the float32 error of the ray."""
    from reflaxman_amd import _lib
    desc = scenes.get_scene(name)
    L = _lib.load()
    eye, at, fov = desc.camera
    view = (C.c_float * 9)()
    L.rfx_camera_view(_lib.farr(eye), _lib.farr(at), view)
    M = np.array(list(view), np.float64).reshape(3, 3)
    rz = float(L.rfx_camera_rz(W, fov))
    o = np.array(eye, np.float64)
    ys, xs = np.mgrid[0:H, 0:W]

    def at_offset(dx, dy):  # Render.cpp:152-153, 183; mmul(view, v): the row-major matrix times the column vector
        loc = np.stack([xs - W / 2.0 + dx, ys - H / 2.0 + dy, np.full(xs.shape, rz)], -1).astype(np.float64)
        return winners(desc, o, loc @ M.T)

    win, ignore = at_offset(0.0, 0.0)
    for dy in (-PROBE, 0.0, PROBE):
        for dx in (-PROBE, 0.0, PROBE):
            if dx or dy:
                ignore = ignore | (at_offset(dx, dy)[0] != win)
    win.setflags(write=False)
    ignore.setflags(write=False)
    return win, ignore


def tiles_of(a, H, W):
    """(tile row, tile column, the tile's pixels of a) over the 8x8 wave tiles of an H x W frame."""
    for ty in range(-(-H // 8)):
        for tx in range(-(-W // 8)):
            yield ty, tx, a[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8]


# ------------------------------------------------------------------ the masks themselves
def test_exact_masks_are_subsets_and_smaller():
    """synth16 160x90 d8, masks built before every launch: every exact word is a subset of its conservative word; words
    0 and 1 hold strictly fewer bits over the frame; a tile that shows only the environment (every pixel of a depth-1
    render equals the colour of a pixel that hits nothing) needs no closest-hit test at all."""
    W, H = 160, 90
    cons, exact = both_masks("synth16", W, H, 8)
    assert cons.shape == exact.shape
    assert not (exact & ~cons).any()
    for w in (0, 1):
        print(f"word {w}: conservative {popcount(cons[..., w])} bits, exact {popcount(exact[..., w])} bits")
        assert popcount(exact[..., w]) < popcount(cons[..., w]), w
    g = Rig(scenes.get_scene("synth16"), W, H, 0)
    _, argb = g.frame(1)
    g.close()
    argb = np.frombuffer(argb, np.uint32).reshape(H, W)
    win, ignore = replay("synth16", W, H)
    sky_colours = set(np.unique(argb[(win < 0) & ~ignore]).tolist())
    assert 1 <= len(sky_colours) <= 2  # no skybox texture: the two colours of the absent texture's checker
    sky = np.isin(argb, sorted(sky_colours))
    n = 0
    for ty, tx, t in tiles_of(sky, H, W):
        if t.all():
            assert exact[ty, tx, 0] == 0, (ty, tx)
            n += 1
    assert n > 0
    # beyond the frame (the launch's padding tiles): nothing to test either
    assert not exact[:, -(-W // 8):, 0].any()


def test_word0_is_the_replayed_winner_set():
    """synth16 64x40: word 0 of every tile holds the bit of every winner the float64 replay finds among the tile's
    pixels it is sure of, and is exactly that set where the tile has no ignored pixel."""
    W, H = 64, 40
    win, ignore = replay("synth16", W, H)
    assert ignore.mean() <= 0.10
    _, exact = both_masks("synth16", W, H, 1)
    sure = 0
    for ty, tx, w in tiles_of(win, H, W):
        ig = ignore[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8]
        want = 0
        for b in np.unique(w[~ig]):
            if b >= 0:
                want |= 1 << int(b)
        got = int(exact[ty, tx, 0])
        assert got & want == want, (ty, tx, hex(got), hex(want))
        if not ig.any():
            assert got == want, (ty, tx, hex(got), hex(want))
            sure += 1
    assert sure > 0


def test_shadow_word_drops_the_tiles_own_triangle():
    """synth16 160x90: a tile whose pixels all lie on ground triangle 0 (by the replay, none ignored) keeps bit 32 in
    its conservative shadow word -- a bundle that starts on the triangle cannot cull it -- and loses it in the exact one."""
    W, H = 160, 90
    win, ignore = replay("synth16", W, H)
    cons, exact = both_masks("synth16", W, H, 8)
    n = 0
    for ty, tx, w in tiles_of(win, H, W):
        if w.shape == (8, 8) and (w == 32).all() and not ignore[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8].any():
            assert cons[ty, tx, 1] >> np.uint64(32) & np.uint64(1) == 1, (ty, tx)
            assert exact[ty, tx, 1] >> np.uint64(32) & np.uint64(1) == 0, (ty, tx)
            n += 1
    assert n > 0


# ------------------------------------------------------------------ no pixel changes
CASES = {
    "partial_tiles": ("synth16", 17, 9, 8, {}),
    "nolight": ("nolight", 40, 24, 4, {}),
    "lights40": ("lights40", 48, 27, 8, {}),
    "planes": ("planes", 40, 24, 6, {}),
    "lanes_ss2": ("synth16", 24, 16, 8, {"ss": 2}),
    "lanes_ss8": ("synth16", 24, 16, 8, {"ss": 8}),
    "additive": ("synth16", 24, 16, 8, {"ss": 1, "additive": True}),
    "strip_rank1of2": ("synth16", 40, 24, 8, {"row_block": 4, "rank": 1, "nranks": 2}),
    "subrange": ("synth16", 40, 24, 8, {"pixel_begin": 40 * 5 + 13, "pixel_end": 40 * 19 + 7}),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_frames_unchanged(case):
    """Three frames of one renderer without masks, with the conservative masks and with the exact ones (both built
    before every launch): the same f32 and ARGB8 bytes, frame by frame.  Jittered frames keep the conservative word 0
    (their hits are not known ahead), so there the two read-backs are equal; every other case must have built masks."""
    name, W, H, depth, kw = CASES[case]
    desc = scenes.get_scene(name)
    frames, masks = [], []
    for mode, exact in ((0, None), (2, 0), (2, 1)):
        g = Rig(desc, W, H, mode, exact)
        frames.append([g.frame(depth, **kw) for _ in range(3)])
        masks.append(g.r.prim_masks().copy())
        g.close()
    assert frames[0] == frames[1], case
    assert frames[0] == frames[2], case
    assert masks[0].size == 0 and masks[1].size > 0 and masks[1].size == masks[2].size
    assert not (masks[2] & ~masks[1]).any()
    if case == "additive":
        assert np.array_equal(masks[1], masks[2])


def test_switch_drops_the_masks_held():
    """A still camera in the default mode (masks built when the view repeats): toggling the switch between two frames
    makes the next frame build its masks again -- the read-back differs -- and the image stays what it was without."""
    W, H, depth = 160, 90, 8
    desc = scenes.get_scene("synth16")
    ref = Rig(desc, W, H, 0)
    want = [ref.frame(depth) for _ in range(4)]
    ref.close()
    g = Rig(desc, W, H, 1)
    got = [g.frame(depth)]
    assert g.r.prim_masks().size == 0  # a view seen once renders without masks
    got.append(g.frame(depth))
    on = g.masks().copy()
    g.r.set_prim_exact(False)
    assert g.r.prim_masks().size == 0
    got.append(g.frame(depth))
    off = g.masks().copy()
    g.r.set_prim_exact(True)
    got.append(g.frame(depth))
    again = g.masks().copy()
    g.close()
    assert got == want
    assert not np.array_equal(on, off)
    assert np.array_equal(on, again)
    cons, exact = both_masks("synth16", W, H, 8)
    assert np.array_equal(off, cons) and np.array_equal(on, exact)
