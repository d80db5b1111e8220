"""Ray batches on the GPU (rfx.h rfx_trace_rays): n Scene::trace calls on rays the caller chose.

Parity is bit equality everywhere: against the committed goldens of the unmodified reference where the rays are a
pinhole frame's, against the per-ray CPU oracle (rays_helpers.oracle_trace) where they are not.
"""
import ctypes as C
import os

import numpy as np
import pytest

import oracle as orc
from helpers import GOLDEN, manifest
from rays_helpers import DEPTH, NRAYS, SEED, incoherent_oracle, incoherent_rays, scene
from reflaxman_amd import _lib, cameras

pytestmark = pytest.mark.gpu

CASES = manifest()["cases"]
RFX_ERR_ARG, RFX_ERR_STATE = -1, -3


def renderer(name, seed=SEED, tri_accel=None):
    """(Renderer with the scene uploaded, its Scene -- kept alive by the caller --, the scene's Camera)."""
    from reflaxman_amd.render import Renderer, build_scene
    s, cam = build_scene(scene(name))
    r = Renderer(sphere_seed=seed, jitter_seed=77)
    if tri_accel is not None:
        r.set_tri_accel(tri_accel)
    r.set_scene(s)
    return r, s, cam


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def trace(r, rays, depth=DEPTH, **kw):
    """The device form on a torch tensor of the rays, results back as numpy (colours, or colours and ARGB words)."""
    import torch
    with torch.cuda.stream(torch.cuda.Stream()):
        out = r.trace_rays(dev(rays), depth, **kw)
        torch.cuda.current_stream().synchronize()
    r.synchronize()  # (the pre-pass's error word)
    if isinstance(out, tuple):
        return out[0].cpu().numpy(), out[1].cpu().numpy().view(np.uint32)
    return out.cpu().numpy()


PINHOLE = [("render_default_160x120_d4", None), ("render_default_7x3_d8", None), ("render_default_1x1_d4", None),
           ("render_lights40_96x54_d8", None), ("render_lights3_160x90_d8", None), ("render_nolight_160x120_d4", None),
           ("render_planes_160x90_d8", None), ("render_planes300_96x54_d8", None),
           ("render_synth16_sky_160x90_d8", None), ("render_stress4096_64x36_d12", None),
           ("render_mesh100_160x90_d8", None), ("render_mesh100_160x90_d8", 1)]


@pytest.mark.parametrize("key,tri_accel", PINHOLE)
def test_pinhole_replay_equals_the_golden_frame(key, tri_accel):
    """cameras.pinhole_rays of a golden's camera, traced with its seed and depth, is the reference's frame: floats and
    ARGB words, as an 8x8-tiled raster and as a linear batch.  Between them the cases take every CFG bit, partial
    tiles and waves (7x3, 1x1, 90 and 54 rows) and a W that is no multiple of 4."""
    c = CASES[key]
    g = np.load(os.path.join(GOLDEN, key + ".npz"))
    W, H = c["W"], c["H"]
    r, s, cam = renderer(c["scene"], c["sphere_seed"], tri_accel)
    rays = cameras.pinhole_rays(tuple(cam.eye), cam.view, cam.fov, W, H)
    for rw in (W, 0):
        r.set_rng(c["sphere_seed"], 77)
        rgb, argb = trace(r, rays, c["depth"], raster_width=rw, argb=True)
        assert rgb.reshape(H, W, 3).tobytes() == g["rgb"].tobytes(), (key, rw)
        assert np.array_equal(argb.reshape(H, W), g["argb"]), (key, rw)
    r.close()


@pytest.mark.parametrize("name,tri_accel", [("default", None), ("stress4096", None), ("planes300", None), ("mesh100", 1)])
def test_incoherent_rays_equal_the_per_ray_oracle(name, tri_accel):
    """357 rays with nothing in common -- origins all over the scene's box, some on or inside objects, lengths from
    1e-3 to 1e3 -- each equal to its Scene::trace on the CPU; the stats kernel gives the same colours and the oracle's
    ray and segment counts."""
    import torch
    rays = incoherent_rays(name)
    want, _, ocnt = incoherent_oracle(name)
    r, s, cam = renderer(name, SEED, tri_accel)
    for rw in (0, 24):
        r.set_rng(SEED, 77)
        got = trace(r, rays, raster_width=rw)
        bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))
        assert bad.size == 0, (name, rw, bad[:8].tolist(), got[bad[:2]].tolist(), want[bad[:2]].tolist())
    r.set_rng(SEED, 77)
    cnt = torch.zeros(_lib.RFX_NCOUNTERS, dtype=torch.int64, device="cuda")
    got = trace(r, rays, counters=cnt)
    assert got.tobytes() == want.tobytes(), name
    gc = cnt.cpu().numpy().view(np.uint64)
    for k in ("rays", "segments"):
        i = list(orc.COUNTER_NAMES).index(k)
        assert int(gc[i]) == int(ocnt[i]), (name, k, int(gc[i]), int(ocnt[i]))
    assert int(gc[list(orc.COUNTER_NAMES).index("rays")]) == NRAYS
    r.close()


@pytest.mark.parametrize("prepass", [1, 0])
def test_stream_continuity(prepass):
    """Two batches equal one; the sphere stream stands n accepted triples on and the jitter stream where it was; a
    frame rendered afterwards is the oracle's frame from that state; the batch takes the pre-pass an unsplit frame
    launch of its size would."""
    from reflaxman_amd.render import make_frame
    name = "default"
    rays = incoherent_rays(name)
    want, end, _ = incoherent_oracle(name)
    assert end == orc.rand_dirs(SEED, NRAYS)[1]
    r, s, cam = renderer(name)
    r.set_rng_prepass(prepass)
    a = trace(r, rays[:100])
    form_a = r.prepass_form()
    b = trace(r, rays[100:])
    assert np.concatenate([a, b]).tobytes() == want.tobytes()
    assert r.get_rng() == (end, 77)
    # what a one-device unsplit frame launch of that many traces takes: the cycle table by default, else the one-pass
    # kernel of small launches
    assert (form_a, r.prepass_form()) == ((1, 1) if prepass else (2, 2))  # (100 and 257 traces: one block each)
    W, H, depth = 160, 120, 4
    img = np.zeros((H, W, 3), np.float32)
    f = make_frame(cam, W, H, depth, 1)
    _lib.check(_lib.load().rfx_render_frame_host(r._h, C.byref(f), _lib.fptr(img), None, None))
    assert (r.prepass_form() == 1) == bool(prepass)
    o = orc.OracleRender(scene(name), end, 0)
    o.set_image_size(W, H)
    o.render(depth, 1)
    assert img.tobytes() == o.image.tobytes()
    assert r.get_rng() == (o.sphere_seed.value, 77)
    r.close()


def test_sizes_and_splitting():
    """Batches of 1, 63, 64 and 65 rays are prefixes of the 357-ray result; with the launch limit at its smallest the
    batch runs as one launch per wave (linear) or per tile row (raster) and no output changes."""
    name = "default"
    rays = incoherent_rays(name)
    want = incoherent_oracle(name)[0]
    r, s, cam = renderer(name)
    for n in (1, 63, 64, 65):
        for rw in (0, 8):
            r.set_rng(SEED, 77)
            assert trace(r, rays[:n], raster_width=rw).tobytes() == want[:n].tobytes(), (n, rw)
    r.set_launch_traces(1)
    for rw in (0, 8, 24):
        r.set_rng(SEED, 77)
        rgb, argb = trace(r, rays, raster_width=rw, argb=True)
        assert rgb.tobytes() == want.tobytes(), rw
        assert np.array_equal(argb, orc.argb_of(want)), rw
        assert r.get_rng()[0] == incoherent_oracle(name)[1]
    r.close()


def test_errors():
    import torch
    from reflaxman_amd.render import Renderer, make_frame
    L = _lib.load()
    name = "default"
    rays = dev(incoherent_rays(name)[:64])
    rgb = torch.zeros((64, 3), dtype=torch.float32, device="cuda")
    img = torch.zeros(16 * 12 * 3, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()  # the renderer's own stream is not ordered with torch's
    p = lambda t: C.c_void_p(t.data_ptr())
    bare = Renderer(sphere_seed=SEED)
    assert L.rfx_trace_rays(bare._h, p(rays), 64, DEPTH, 0, p(rgb), None, None, None) == RFX_ERR_STATE  # no scene
    bare.close()
    r, s, cam = renderer(name)
    assert L.rfx_trace_rays(r._h, p(rays), 0, DEPTH, 0, p(rgb), None, None, None) == RFX_ERR_ARG
    assert L.rfx_trace_rays(r._h, None, 64, DEPTH, 0, p(rgb), None, None, None) == RFX_ERR_ARG
    assert L.rfx_trace_rays(r._h, p(rays), 64, DEPTH, 0, None, None, None, None) == RFX_ERR_ARG
    assert L.rfx_trace_rays(r._h, p(rays), 64, 0, 0, p(rgb), None, None, None) == RFX_ERR_ARG
    assert L.rfx_trace_rays(r._h, p(rays), 64, -1, 0, p(rgb), None, None, None) == RFX_ERR_ARG
    assert L.rfx_trace_rays(None, p(rays), 64, DEPTH, 0, p(rgb), None, None, None) == RFX_ERR_ARG
    host = np.zeros((64, 3), np.float32)
    assert L.rfx_trace_rays_host(r._h, None, 64, DEPTH, 0, _lib.fptr(host), None, None) == RFX_ERR_ARG
    assert r.get_rng() == (SEED, 77)  # a refused call moves no stream
    # a rewind undoes an rfx_render_frame only
    f = make_frame(cam, 16, 12, 4, 1)
    r.render_frame(f, img.data_ptr())
    assert L.rfx_trace_rays(r._h, p(rays), 64, DEPTH, 0, p(rgb), None, None, None) == 0
    assert L.rfx_frame_rng_rewind(r._h) == RFX_ERR_STATE
    # no batch while an emitted frame awaits its trace
    bps = C.c_uint64()
    _lib.check(L.rfx_frame_rng_blocks(r._h, C.byref(f), 1, C.byref(bps)))
    counts = torch.zeros(bps.value, dtype=torch.int32, device="cuda")
    _lib.check(L.rfx_frame_rng_count(r._h, C.byref(f), 0, 1, p(counts), None))
    _lib.check(L.rfx_frame_rng_emit(r._h, C.byref(f), 1, p(counts), None, None))
    assert L.rfx_trace_rays(r._h, p(rays), 64, DEPTH, 0, p(rgb), None, None, None) == RFX_ERR_STATE
    _lib.check(L.rfx_frame_rng_discard(r._h))
    assert L.rfx_trace_rays(r._h, p(rays), 64, DEPTH, 0, p(rgb), None, None, None) == 0
    r.synchronize()
    r.close()


def test_host_form_equals_device_form():
    name = "stress4096"
    rays = incoherent_rays(name)
    r, s, cam = renderer(name)
    d_rgb, d_argb = trace(r, rays, argb=True)
    r.set_rng(SEED, 77)
    cnt = np.zeros(_lib.RFX_NCOUNTERS, np.uint64)
    h_rgb, h_argb = r.trace_rays(rays, DEPTH, argb=True)
    assert h_rgb.tobytes() == d_rgb.tobytes() and np.array_equal(h_argb, d_argb)
    assert r.get_rng()[0] == incoherent_oracle(name)[1]
    r.set_rng(SEED, 77)
    assert r.trace_rays(rays, DEPTH, raster_width=16, counters=cnt).tobytes() == d_rgb.tobytes()
    assert int(cnt[list(orc.COUNTER_NAMES).index("rays")]) == NRAYS
    r.close()


def test_render_trace_rays_on_the_scene_owner():
    """Render.traceRays: origins and directions in, colours out, on the object's own scene and stream state."""
    from reflaxman_amd.render import Render, build_scene
    name = "default"
    rays = incoherent_rays(name)[:65]
    r = Render(sphere_seed=SEED, jitter_seed=77, load_default_scene=False)
    r.scene, r.camera = build_scene(scene(name))
    got = r.traceRays(rays[:, 0:3], rays[:, 3:6], DEPTH)
    assert got.tobytes() == incoherent_oracle(name)[0][:65].tobytes()
    with pytest.raises(ValueError):
        r.traceRays(rays[:, 0:3], rays[:, 3:6], 0)
    r.close()
