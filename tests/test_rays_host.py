"""Ray batches, the part that needs no GPU: the camera models' rays and the ABI's new entries."""
import os
import re

import numpy as np

import oracle as orc
from rays_helpers import oracle_trace, scene
from reflaxman_amd import _lib, cameras

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pinhole_rays_reproduce_the_oracle_frame():
    """The per-ray oracle over pinhole_rays' rays is the oracle's own frame, pixel for pixel, and ends on the same
    stream state: the rays are the pixel loop's bit for bit (a different ray gives a different float somewhere in 192
    depth-6 traces), and the 1 x 1 oracle is Scene::trace."""
    desc = scene("default")
    W, H, depth, seed = 16, 12, 6, 1350490027
    o = orc.OracleRender(desc, seed, 0)
    o.set_image_size(W, H)
    o.render(depth, 1)
    eye, at, fov = desc.camera
    rays = cameras.pinhole_rays(eye, orc.camera_view(eye, at), fov, W, H)
    assert rays.shape == (W * H, 6) and rays.dtype == np.float32
    rgb, end = oracle_trace(desc, rays, depth, seed)
    assert rgb.reshape(H, W, 3).tobytes() == o.image.tobytes()
    assert end == o.sphere_seed.value


def test_pinhole_rz_with_and_without_the_library():
    L = _lib.load()
    saved = _lib._lib
    try:
        for W, fov in ((16, 1.05), (3840, 1.05), (7, 0.3), (1, 2.5)):
            _lib._lib = L
            a = cameras.camera_rz(W, fov)
            _lib._lib = None
            b = cameras.camera_rz(W, fov)
            assert a.dtype == np.float32 and a.tobytes() == b.tobytes(), (W, fov)
    finally:
        _lib._lib = saved


def test_equirect_rays_shape_poles_and_seam():
    W, H = 16, 8
    eye = (1.0, 2.0, -3.0)
    r = cameras.equirect_rays(eye, W, H)
    assert r.shape == (W * H, 6) and r.dtype == np.float32
    assert (r[:, 0:3] == np.array(eye, np.float32)).all()
    d = r[:, 3:6].astype(np.float64).reshape(H, W, 3)
    assert np.allclose(np.linalg.norm(d, axis=2), 1.0, atol=1e-6)
    assert not (r[:, 3:6] == 0).any()  # pixel centres: no ray along an axis or at a pole
    # row 0 is the bottom, the last row the top; each half a pixel's latitude from its pole
    lat = np.arcsin(d[:, :, 1])
    assert np.allclose(lat[0], -np.pi / 2 + np.pi / (2 * H)) and np.allclose(lat[-1], np.pi / 2 - np.pi / (2 * H))
    # the rows are symmetric about the equator, the columns about the +z meridian
    assert np.allclose(d[::-1, :, 1], -d[:, :, 1]) and np.allclose(d[:, ::-1, 0], -d[:, :, 0])
    # longitude grows with x from the -z seam: the middle columns straddle +z, the first and last sit half a pixel
    # either side of -z, a whole pixel (2 pi / W) apart across the seam
    lon = np.arctan2(d[H // 2, :, 0], d[H // 2, :, 2])
    assert np.allclose(np.diff(lon), 2 * np.pi / W)
    assert np.isclose(lon[0], -np.pi + np.pi / W) and np.isclose(lon[-1], np.pi - np.pi / W)
    assert d[H // 2, W // 2 - 1, 2] > 0 and d[H // 2, W // 2, 2] > 0 and d[H // 2, 0, 2] < 0


def test_abi_version_5_and_ray_entry_points():
    text = open(os.path.join(ROOT, "include", "rfx.h")).read()
    assert re.search(r"^#define RFX_ABI_VERSION 5$", text, re.M)
    assert _lib.RFX_ABI_VERSION == 5
    L = _lib.load()
    assert L.rfx_abi_version() == 5
    bound = {n for n, _, _ in _lib.SIGNATURES}
    for name in ("rfx_trace_rays", "rfx_trace_rays_host"):
        assert re.search(r"\bint %s\(" % name, text) and hasattr(L, name) and name in bound, name
